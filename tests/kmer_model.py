"""The contract of the sketches from sequences in pure Python (include/mvs_hip.h, "sketches from sequences"): MurmurHash3_x64_128's
first word, the canonical k-mer, the sketch of a byte string.  The tests of mvs_kmer_hash, mvs_hash_set_from_sequences and
sketch_sequences take every expected value from here and from nowhere else."""
import numpy as np

M64 = (1 << 64) - 1
C1, C2 = 0x87C37B91114253D5, 0x4CF5AD432745937F
_COMP = {65: 84, 67: 71, 71: 67, 84: 65}   # A<->T, C<->G
_BASES = b"ACGTacgt"


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _fmix(k):
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    return k ^ (k >> 33)


def murmur3_h1(data, seed=0):
    """first 64-bit word of MurmurHash3_x64_128(data, seed)"""
    data = bytes(data)
    n = len(data)
    h1 = h2 = seed & 0xFFFFFFFF
    for b in range(n // 16):
        k1 = int.from_bytes(data[16 * b:16 * b + 8], "little")
        k2 = int.from_bytes(data[16 * b + 8:16 * b + 16], "little")
        k1 = (k1 * C1) & M64; k1 = _rotl(k1, 31); k1 = (k1 * C2) & M64; h1 ^= k1
        h1 = _rotl(h1, 27); h1 = (h1 + h2) & M64; h1 = (h1 * 5 + 0x52DCE729) & M64
        k2 = (k2 * C2) & M64; k2 = _rotl(k2, 33); k2 = (k2 * C1) & M64; h2 ^= k2
        h2 = _rotl(h2, 31); h2 = (h2 + h1) & M64; h2 = (h2 * 5 + 0x38495AB5) & M64
    tail = data[16 * (n // 16):]
    if len(tail) > 8:
        k2 = int.from_bytes(tail[8:], "little")
        k2 = (k2 * C2) & M64; k2 = _rotl(k2, 33); k2 = (k2 * C1) & M64; h2 ^= k2
    if len(tail) > 0:
        k1 = int.from_bytes(tail[:8], "little")
        k1 = (k1 * C1) & M64; k1 = _rotl(k1, 31); k1 = (k1 * C2) & M64; h1 ^= k1
    h1 ^= n; h2 ^= n
    h1 = (h1 + h2) & M64; h2 = (h2 + h1) & M64
    h1 = _fmix(h1); h2 = _fmix(h2)
    return (h1 + h2) & M64


def max_hash(scaled):
    if scaled < 1:
        raise ValueError("scaled < 1")
    return M64 if scaled == 1 else int(18446744073709551616.0 / float(scaled))


def revcomp(kmer):
    return bytes(_COMP[b] for b in reversed(bytes(kmer).upper()))


def canonical(kmer):
    """the smaller of the upper-cased k-mer and its reverse complement, or None if a byte is a break"""
    kmer = bytes(kmer)
    if any(b not in _BASES for b in kmer):
        return None
    fw = kmer.upper()
    rc = revcomp(fw)
    return fw if fw <= rc else rc


def kmer_hash(kmer, seed=42):
    c = canonical(kmer)
    return None if c is None else murmur3_h1(c, seed)


def kept_values(sample, ksize=31, seed=42, maxh=M64, memo=None):
    """-> (valid positions, the kept values in position order, duplicates included).  memo: a dict the caller keeps for ONE
    (ksize, seed), upper-cased k-mer -> value, so that samples which share most of their k-mers are hashed once"""
    sample = bytes(sample)
    is_base = [b in _BASES for b in sample]
    up = sample.upper()
    run, valid, kept = 0, 0, []
    if memo is None:
        memo = {}
    for i in range(len(sample)):
        run = run + 1 if is_base[i] else 0
        if run >= ksize:
            valid += 1
            fw = up[i - ksize + 1:i + 1]
            h = memo.get(fw)
            if h is None:
                rc = revcomp(fw)
                h = murmur3_h1(fw if fw <= rc else rc, seed)
                memo[fw] = h
            if h <= maxh:
                kept.append(h)
    return valid, kept


def sketch(sample, ksize=31, seed=42, maxh=M64):
    """the sketch of one sample: ascending distinct values"""
    return sorted(set(kept_values(sample, ksize, seed, maxh)[1]))


def sketch_csr(samples, ksize=31, seed=42, maxh=M64):
    """-> (hashes uint64, offsets int64) of the sketches of several samples"""
    lists = [sketch(s, ksize, seed, maxh) for s in samples]
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    if lists:
        np.cumsum([len(x) for x in lists], out=offsets[1:])
    flat = [v for x in lists for v in x]
    return np.array(flat, dtype=np.uint64), offsets


def random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes())
