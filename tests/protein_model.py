"""The contract of the protein sketches in pure Python (include/mvs_hip.h, "protein sketches"): residues and breaks, the three
alphabets, the standard genetic code, the six reading frames, the sketch of a byte string.  The tests of mvs_aa_hash,
mvs_translate_codon, mvs_hash_set_from_residues and sketch_proteins take every expected value from here and from nowhere else;
the hash itself is tests/kmer_model.py's murmur3_h1."""
import numpy as np

from kmer_model import M64, max_hash, murmur3_h1  # noqa: F401  (max_hash: re-exported for the tests)

LETTERS = b"ACDEFGHIKLMNPQRSTVWY"
STOP = ord("*")
DAYHOFF = {"a": "C", "b": "AGPST", "c": "DENQ", "d": "HKR", "e": "ILMV", "f": "FWY"}
HP = {"h": "AFGILMPVWY", "p": "CDEHKNQRST"}
ALPHABETS = ("protein", "dayhoff", "hp")
DEFAULT_KSIZE = {"protein": 10, "dayhoff": 16, "hp": 42}
CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
_TCAG = {ord(b): i for i, b in enumerate("TCAG")}
_TCAG.update({ord(b): i for i, b in enumerate("tcag")})
_COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}
_BASES = b"ACGTacgt"


def _encoder(alphabet):
    """byte -> the byte the hash reads, for the residues only"""
    enc = {}
    for L in LETTERS:
        c = chr(L)
        if alphabet == "protein":
            e = L
        elif alphabet == "dayhoff":
            e = ord(next(k for k, v in DAYHOFF.items() if c in v))
        elif alphabet == "hp":
            e = ord(next(k for k, v in HP.items() if c in v))
        else:
            raise ValueError(alphabet)
        enc[L] = e
        enc[ord(c.lower())] = e
    enc[STOP] = STOP
    return enc


ENCODERS = {a: _encoder(a) for a in ALPHABETS}


def encode(kmer, alphabet="protein"):
    """the bytes the hash reads for a k-mer of residues, or None if a byte is a break"""
    enc = ENCODERS[alphabet]
    out = bytearray()
    for b in bytes(kmer):
        if b not in enc:
            return None
        out.append(enc[b])
    return bytes(out)


def aa_hash(kmer, alphabet="protein", seed=42):
    e = encode(kmer, alphabet)
    return None if e is None else murmur3_h1(e, seed)


def translate_codon(codon):
    """the residue (one upper-case byte or '*') of three bases, or None if one of them is no base"""
    codon = bytes(codon)
    assert len(codon) == 3
    if any(b not in _TCAG for b in codon):
        return None
    x, y, z = (_TCAG[b] for b in codon)
    return CODE[16 * x + 4 * y + z].encode()


def translate(dna):
    """a run of bases codon by codon; a trailing partial codon is dropped"""
    dna = bytes(dna)
    return b"".join(translate_codon(dna[i:i + 3]) for i in range(0, len(dna) - 2, 3))


def revcomp(dna):
    return bytes(_COMP[b] for b in reversed(bytes(dna).upper()))


def base_runs(sample):
    """the maximal runs of bases of a byte string"""
    runs, cur = [], bytearray()
    for b in bytes(sample):
        if b in _BASES:
            cur.append(b)
        else:
            if cur:
                runs.append(bytes(cur))
            cur = bytearray()
    if cur:
        runs.append(bytes(cur))
    return runs


def six_frames(sample):
    """the translated frames of every maximal run of bases: the run and its reverse complement at offsets 0, 1, 2"""
    out = []
    for run in base_runs(sample):
        for strand in (run.upper(), revcomp(run)):
            for off in range(3):
                out.append(translate(strand[off:]))
    return out


def protein_values(sample, ksize, alphabet="protein", seed=42, maxh=M64, memo=None):
    """input kind protein -> (hashed k-mers, the kept values in position order, duplicates included)"""
    sample = bytes(sample)
    enc = ENCODERS[alphabet]
    if memo is None:
        memo = {}
    coded = bytes(enc.get(b, 0) for b in sample)
    run, n, kept = 0, 0, []
    for i in range(len(coded)):
        run = run + 1 if coded[i] else 0
        if run >= ksize:
            n += 1
            w = coded[i - ksize + 1:i + 1]
            h = memo.get(w)
            if h is None:
                h = memo[w] = murmur3_h1(w, seed)
            if h <= maxh:
                kept.append(h)
    return n, kept


def translate_values(sample, ksize, alphabet="protein", seed=42, maxh=M64, memo=None):
    """input kind translate, as the contract states it: the six frames of every run, every window of ksize residues"""
    if memo is None:
        memo = {}
    n, kept = 0, []
    for frame in six_frames(sample):
        m, k = protein_values(frame, ksize, alphabet, seed, maxh, memo)
        n += m
        kept += k
    return n, kept


def translate_values_by_window(sample, ksize, alphabet="protein", seed=42, maxh=M64):
    """the equivalent statement: every window of 3 * ksize bases gives two values, its codons read forward and the codons of
    its reverse complement"""
    sample = bytes(sample)
    w = 3 * ksize
    n, kept = 0, []
    for p in range(len(sample) - w + 1):
        win = sample[p:p + w]
        if any(b not in _BASES for b in win):
            continue
        for strand in (win.upper(), revcomp(win)):
            h = aa_hash(translate(strand), alphabet, seed)
            assert h is not None
            n += 1
            if h <= maxh:
                kept.append(h)
    return n, kept


def values(sample, ksize, alphabet="protein", translate_dna=False, seed=42, maxh=M64, memo=None):
    return (translate_values if translate_dna else protein_values)(sample, ksize, alphabet, seed, maxh, memo)


def call_model(samples, ksize, alphabet="protein", translate_dna=False, seed=42, maxh=M64):
    """what one library call gives: hashes uint64 / offsets int64 of the sketches, hashed k-mers and kept values per sample"""
    memo = {}
    lists, kmers, kept = [], [], []
    for s in samples:
        n, k = values(s, ksize, alphabet, translate_dna, seed, maxh, memo)
        lists.append(sorted(set(k)))
        kmers.append(n)
        kept.append(len(k))
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    if lists:
        np.cumsum([len(x) for x in lists], out=offsets[1:])
    return {"hashes": np.array([v for x in lists for v in x], dtype=np.uint64), "offsets": offsets, "kmers": kmers, "kept": kept,
            "bytes": sum(len(bytes(s)) for s in samples), "lists": lists}


def random_residues(rng, n, letters=LETTERS):
    return bytes(rng.choice(np.frombuffer(bytes(letters), dtype=np.uint8), size=n).tobytes())


def random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes())
