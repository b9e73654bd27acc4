"""CPU: the contract of the protein sketches on the host -- the anchors that do not depend on this code (the two public murmur
digests, the 64-letter table of the standard genetic code, one translated sequence); mvs_translate_codon for all 64 codons in
both cases and a non-base in each place; mvs_aa_hash equals the model (tests/protein_model.py) for every ksize 1 .. 64 in the
three alphabets, in lower and mixed case, with the stop, with a break at every position, and its refusals; the dayhoff and hp
classes partition the 20 letters; the model's six-frame statement equals its own per-window statement.  No device needed."""
import itertools

import numpy as np
import pytest

import metagenome_vector_sketches_amd as pkg
import protein_model as pm

TABLE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
BREAKS = (b"X", b"B", b"Z", b"J", b"U", b"O", b"-", b"\n", b"\x00", b"\xff", b"x", b"b", b" ", b"1")


def test_the_anchors():
    assert pm.murmur3_h1(b"hello", 0) == 0xCBD8A7B341BD9B02
    assert pm.murmur3_h1(b"The quick brown fox jumps over the lazy dog", 0) == 0xE34BBC7BBC071B6C
    assert pm.CODE == TABLE and len(TABLE) == 64
    # a few codons everybody knows, through the index rule T, C, A, G = 0, 1, 2, 3
    for codon, aa in (("ATG", "M"), ("TGG", "W"), ("TAA", "*"), ("TAG", "*"), ("TGA", "*"), ("TTT", "F"), ("GGG", "G"), ("AAA", "K")):
        assert pm.translate_codon(codon.encode()) == aa.encode()
    assert pm.translate(b"ATGGCCATTGTAATGGGCCGCTGAAAGGGTGCCCGATAG") == b"MAIVMGR*KGAR*"
    assert "".join(pkg.translate_codon(b"ATGGCCATTGTAATGGGCCGCTGAAAGGGTGCCCGATAG"[i:i + 3]) for i in range(0, 39, 3)) == "MAIVMGR*KGAR*"


def test_translate_codon_all_64_in_both_cases_and_a_non_base_in_each_place():
    for i, (x, y, z) in enumerate(itertools.product("TCAG", repeat=3)):
        codon = x + y + z
        assert pkg.translate_codon(codon) == TABLE[i] == pm.translate_codon(codon.encode()).decode()
        assert pkg.translate_codon(codon.lower()) == TABLE[i]
        assert pkg.translate_codon(codon.encode()) == TABLE[i]
        assert pkg.translate_codon(x.lower() + y + z.lower()) == TABLE[i]
        for place in range(3):
            for bad in "NU-RYn\n\x00":
                broken = codon[:place] + bad + codon[place + 1:]
                assert pkg.translate_codon(broken) is None and pm.translate_codon(broken.encode("latin-1")) is None
    assert pkg.translate_codon(b"AC\xff") is None
    with pytest.raises(ValueError):
        pkg.translate_codon("AC")


def test_the_classes_partition_the_20_letters():
    letters = sorted(chr(b) for b in pm.LETTERS)
    assert len(letters) == 20 and len(set(letters)) == 20
    for classes in (pm.DAYHOFF, pm.HP):
        members = sorted("".join(classes.values()))
        assert members == letters
    assert pm.DAYHOFF == {"a": "C", "b": "AGPST", "c": "DENQ", "d": "HKR", "e": "ILMV", "f": "FWY"}
    assert pm.HP == {"h": "AFGILMPVWY", "p": "CDEHKNQRST"}
    # the library's classes, read off its hashes of single residues
    for alphabet, classes in (("dayhoff", pm.DAYHOFF), ("hp", pm.HP)):
        for code, members in classes.items():
            for m in members:
                assert pkg.aa_hash(m, alphabet) == pm.murmur3_h1(code.encode(), 42) == pkg.aa_hash(m.lower(), alphabet)
    for alphabet in pm.ALPHABETS:
        assert pkg.aa_hash("*", alphabet) == pm.murmur3_h1(b"*", 42)
    for L in letters:
        assert pkg.aa_hash(L, "protein") == pm.murmur3_h1(L.encode(), 42)


@pytest.mark.parametrize("alphabet", pm.ALPHABETS)
@pytest.mark.parametrize("ksize", range(1, 65))
def test_aa_hash_equals_the_model(ksize, alphabet):
    rng = np.random.default_rng(1000 * pm.ALPHABETS.index(alphabet) + ksize)
    for trial in range(4):
        kmer = pm.random_residues(rng, ksize, pm.LETTERS + b"*" if trial == 3 else pm.LETTERS)
        seed = 42 if trial < 2 else int(rng.integers(0, 1 << 32))
        want = pm.aa_hash(kmer, alphabet, seed)
        assert want is not None and pkg.aa_hash(kmer, alphabet, seed) == want
        assert pkg.aa_hash(kmer.lower(), alphabet, seed) == want
        assert pkg.aa_hash(kmer.decode(), alphabet, seed) == want
        mixed = bytes(b | 0x20 if i % 2 and b != pm.STOP else b for i, b in enumerate(kmer))
        assert pkg.aa_hash(mixed, alphabet, seed) == want
    kmer = pm.random_residues(rng, ksize)
    with_stop = kmer[:ksize // 2] + b"*" + kmer[ksize // 2 + 1:]
    assert pkg.aa_hash(with_stop, alphabet) == pm.aa_hash(with_stop, alphabet) is not None
    for pos in range(ksize):
        for brk in BREAKS:
            broken = kmer[:pos] + brk + kmer[pos + 1:]
            assert pm.aa_hash(broken, alphabet) is None and pkg.aa_hash(broken, alphabet) is None


def test_aa_hash_defaults_and_refusals():
    assert pkg.aa_hash(b"MAIVMGRKGA") == pm.aa_hash(b"MAIVMGRKGA", "protein", 42) != pm.aa_hash(b"MAIVMGRKGA", "protein", 0)
    assert pkg.aa_hash(b"MAIVMGRKGA", "hp") == pm.murmur3_h1(b"hhhhhhpphh", 42)
    assert pkg.aa_hash(b"MAIVMGRKGA", "dayhoff") == pm.murmur3_h1(b"ebeeebddbb", 42)
    for bad in (b"", b"A" * 65):
        with pytest.raises(pkg.MvsError) as e:
            pkg.aa_hash(bad)
        assert e.value.code == pkg._capi.MVS_E_INVALID
    with pytest.raises(ValueError):
        pkg.aa_hash(b"ACD", "dna")
    lib = pkg.load_library()
    import ctypes
    h, valid = ctypes.c_uint64(), ctypes.c_int()
    for alphabet in (-1, 3):
        assert lib.mvs_aa_hash(b"ACD", 3, alphabet, 42, ctypes.byref(h), ctypes.byref(valid)) == pkg._capi.MVS_E_INVALID
    assert lib.mvs_aa_hash(None, 3, 0, 42, ctypes.byref(h), ctypes.byref(valid)) == pkg._capi.MVS_E_INVALID
    assert lib.mvs_aa_hash(b"ACD", 3, 0, 42, None, ctypes.byref(valid)) == pkg._capi.MVS_E_INVALID
    assert lib.mvs_translate_codon(None, ctypes.create_string_buffer(1), ctypes.byref(valid)) == pkg._capi.MVS_E_INVALID


@pytest.mark.parametrize("ksize", [1, 2, 5, 11])
def test_six_frames_equal_the_windows(ksize):
    rng = np.random.default_rng(7 + ksize)
    dna = bytearray(pm.random_bases(rng, 700))
    for at in rng.integers(0, len(dna), size=6):
        dna[at] = ord("N")
    dna[100:103] = b"\nnN"
    dna[300:340] = bytes(dna[300:340]).lower()
    # runs shorter than a window, of exactly one window, and one byte longer
    w = 3 * ksize
    dna += b"N" + pm.random_bases(rng, w - 1) + b"N" + pm.random_bases(rng, w) + b"-" + pm.random_bases(rng, w + 1)
    dna = bytes(dna)
    for alphabet in pm.ALPHABETS:
        n1, k1 = pm.translate_values(dna, ksize, alphabet)
        n2, k2 = pm.translate_values_by_window(dna, ksize, alphabet)
        assert n1 == n2 > 0 and sorted(k1) == sorted(k2)
    # a level: the same multiset below it
    level = pm.max_hash(4)
    n1, k1 = pm.translate_values(dna, ksize, "protein", maxh=level)
    n2, k2 = pm.translate_values_by_window(dna, ksize, "protein", maxh=level)
    assert n1 == n2 and sorted(k1) == sorted(k2) and 0 < len(k1) < n1


def test_a_sequence_and_its_reverse_complement_translate_to_the_same_sketch():
    rng = np.random.default_rng(3)
    dna = pm.random_bases(rng, 400)
    a = pm.call_model([dna], 7, "protein", True)
    b = pm.call_model([pm.revcomp(dna)], 7, "protein", True)
    assert a["lists"] == b["lists"] and a["kmers"] == b["kmers"] == [2 * (400 - 21 + 1)]
