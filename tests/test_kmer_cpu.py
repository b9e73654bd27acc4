"""CPU: the contract of the sketches from sequences on the host -- the model (tests/kmer_model.py) gives the two digests everybody
quotes for MurmurHash3_x64_128; mvs_kmer_hash equals the model for every ksize on random k-mers, their reverse complements,
lower case and a break at every position; mvs_kmer_max_hash equals the formula with the values written out; the parser's
self-test passes.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

import kmer_model as km
import metagenome_vector_sketches_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metagenome_vector_sketches_amd", "bin")


def test_model_gives_the_anchor_digests():
    assert km.murmur3_h1(b"hello", 0) == 0xCBD8A7B341BD9B02
    assert km.murmur3_h1(b"The quick brown fox jumps over the lazy dog", 0) == 0xE34BBC7BBC071B6C


@pytest.mark.parametrize("ksize", range(1, 33))
def test_kmer_hash_equals_the_model(ksize):
    rng = np.random.default_rng(100 + ksize)
    for trial in range(6):
        kmer = km.random_bases(rng, ksize)
        seed = 42 if trial < 3 else int(rng.integers(0, 1 << 32))
        want = km.kmer_hash(kmer, seed)
        assert want is not None and pkg.kmer_hash(kmer, seed) == want
        assert pkg.kmer_hash(km.revcomp(kmer), seed) == want                  # a k-mer and its reverse complement: one value
        assert pkg.kmer_hash(kmer.lower(), seed) == want
        assert pkg.kmer_hash(kmer.decode(), seed) == want
        mixed = bytes(b | 0x20 if i % 2 else b for i, b in enumerate(kmer))
        assert pkg.kmer_hash(mixed, seed) == want
    kmer = km.random_bases(rng, ksize)
    for pos in range(ksize):
        for brk in (b"N", b"\n", b"\x00", b"\xff", b"R", b"n", b"U", b"@"):
            broken = kmer[:pos] + brk + kmer[pos + 1:]
            assert km.kmer_hash(broken) is None and pkg.kmer_hash(broken) is None


def test_kmer_hash_default_seed_is_42_and_sizes_are_checked():
    assert pkg.kmer_hash(b"ACGTTGCA") == km.kmer_hash(b"ACGTTGCA", 42) != km.kmer_hash(b"ACGTTGCA", 0)
    assert pkg.kmer_hash(b"ACGT") == pkg.kmer_hash(b"ACGT", 42)               # a palindrome is its own reverse complement
    for bad in (b"", b"A" * 33):
        with pytest.raises(pkg.MvsError) as e:
            pkg.kmer_hash(bad)
        assert e.value.code == pkg._capi.MVS_E_INVALID


def test_kmer_max_hash_values():
    want = {1: 18446744073709551615, 2: 9223372036854775808, 10: 1844674407370955264, 100: 184467440737095520,
            1000: 18446744073709552, 2000: 9223372036854776, 10000: 1844674407370955}
    for scaled, value in want.items():
        assert pkg.kmer_max_hash(scaled) == value == km.max_hash(scaled)
    for scaled in (2, 10, 100, 1000, 2000, 10000):
        assert want[scaled] == int(18446744073709551616.0 / float(scaled))
    for bad in (0, -1):
        with pytest.raises(pkg.MvsError) as e:
            pkg.kmer_max_hash(bad)
        assert e.value.code == pkg._capi.MVS_E_INVALID


def test_parser_selftest_exits_0():
    r = subprocess.run([os.path.join(BIN, "mvs_fasta_selftest")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
