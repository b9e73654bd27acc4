"""What k_kmer_hash does with ONE unit of work, replayed in plain Python on top of tests/kmer_model.py: which positions a thread
owns, what a wave's buffer of kept values holds when it is flushed, and the model of a whole call with the per-position kept
flags that replay needs.  The values themselves come from kmer_model.kept_values and from nowhere else; this module only says
WHERE they lie, so that a test can assert that its input reaches the path it is named for before it runs the kernel."""
import numpy as np

import kmer_model as km

THREADS = 256           # of a workgroup of k_kmer_hash
WAVE = 64
WAVE_BUF = 512          # kept values a wave collects between two flushes


def per_thread(npos, threads=THREADS):
    """R: the consecutive positions a thread of a unit of npos positions owns"""
    return -(-npos // threads)


def unit_sizes(npos, unit):
    """the positions of a sample's units of work, in order"""
    return [min(unit, npos - p0) for p0 in range(0, max(npos, 0), unit)]


def wave_flushes(keep, npos, buf=WAVE_BUF):
    """keep: the kept flag of every position of ONE unit (npos of them) -> [(wave, fill, mid_loop)]: every flush of a wave's
    buffer in the order the wave makes them.  Thread t owns positions t*R .. t*R + R - 1, wave w is threads 64w .. 64w + 63, step
    j ballots one position per lane; the buffer is flushed in the loop when it cannot take the ballot's values, and once more at
    the end when it holds any."""
    assert len(keep) == npos
    R = per_thread(npos)
    out = []
    for w in range(THREADS // WAVE):
        fill = 0
        for j in range(R):
            n = 0
            for lane in range(WAVE):
                p = (WAVE * w + lane) * R + j
                if p < npos and keep[p]:
                    n += 1
            if n:
                if fill + n > buf:
                    out.append((w, fill, True))
                    fill = 0
                fill += n
        if fill:
            out.append((w, fill, False))
    return out


def position_flags(sample, ksize, values, maxh):
    """values: kmer_model.kept_values(sample, ksize, seed, M64)[1], one per valid position -> per position of the sample (len -
    ksize + 1 of them) whether its value is kept at the level maxh"""
    base = [b in b"ACGTacgt" for b in bytes(sample)]
    flags, run, it = [], 0, iter(values)
    for i, b in enumerate(base):
        run = run + 1 if b else 0
        if i >= ksize - 1:
            flags.append(run >= ksize and next(it) <= maxh)
    assert next(it, None) is None, "the walk and kmer_model.kept_values disagree about the valid positions"
    return flags


def call_model(samples, ksize, seed=42, maxh=km.M64, memo=None, flags=True):
    """-> dict of what one sketch_sequences call must give: hashes / offsets (the export), kmers / kept per sample, and with
    flags=True the kept flag of every position of every sample.  One hashing pass per sample, through kmer_model.kept_values."""
    lists, kmers, kept, fl = [], [], [], []
    for s in samples:
        valid, values = km.kept_values(s, ksize, seed, km.M64, memo)
        k = values if maxh == km.M64 else [v for v in values if v <= maxh]
        lists.append(sorted(set(k)))
        kmers.append(valid)
        kept.append(len(k))
        if flags:
            fl.append(position_flags(s, ksize, values, maxh))
            assert sum(fl[-1]) == len(k)
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    if lists:
        np.cumsum([len(x) for x in lists], out=offsets[1:])
    return dict(hashes=np.array([v for x in lists for v in x], dtype=np.uint64), offsets=offsets, kmers=kmers, kept=kept,
                flags=fl if flags else None, bases=sum(len(s) for s in samples))


def call_flushes(model, unit, buf=WAVE_BUF):
    """every flush of a call: [(sample, unit of the sample, wave, fill, mid_loop)]"""
    out = []
    for s, fl in enumerate(model["flags"]):
        p0 = 0
        for u, npos in enumerate(unit_sizes(len(fl), unit)):
            out += [(s, u) + f for f in wave_flushes(fl[p0:p0 + npos], npos, buf)]
            p0 += npos
    return out


def some_flush_straddles(fills, cap):
    """True if, in WHATEVER order the flushes of these fills reach the list's cursor, one of them starts below cap and ends
    above it: cap is below their sum and is no sum of a subset of them (the cursor only ever stands at such a sum)"""
    if cap >= sum(fills):
        return False
    reach = 1
    for f in fills:
        reach |= reach << f
    return not (reach >> cap) & 1
