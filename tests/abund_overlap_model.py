"""The abundance-weighted overlaps of include/mvs_hip.h ("abundance-weighted overlaps"), transcribed into pure Python: a sample
is a dict {value: abundance} of Python ints, the integer fields are exact Python ints, the derived measures use `math` on floats
made from whole integers (float(int) rounds to nearest-even whatever the integer's size).  No numpy, no device, no library."""
import math

MASK32 = (1 << 32) - 1
FIELDS = ("inter", "w_row", "w_col", "w_min", "dot_lo", "dot_hi")
MEASURES = ("w_contain_row", "w_contain_col", "bray_curtis", "ruzicka", "cosine", "angular")


def sample(values, weights=None, min_abundance=1, max_abundance=0):
    """values in any order, duplicates welcome, weights aligned (default 1 each) -> {value: summed weight} after the filter of
    mvs_hash_set_create_counted (a sum of 0 counts as absent)"""
    d = {}
    for i, v in enumerate(values):
        d[int(v)] = d.get(int(v), 0) + (1 if weights is None else int(weights[i]))
    return {v: a for v, a in d.items() if a >= max(1, min_abundance) and (max_abundance == 0 or a <= max_abundance)}


def plain(values):
    """a set that carries no abundances: 1 for every value"""
    return {int(v): 1 for v in values}


def overlap(row, col):
    """-> dict of the six integer fields of the cell (row, col)"""
    small, large = (row, col) if len(row) <= len(col) else (col, row)
    o = dict.fromkeys(FIELDS, 0)
    for h in small:
        if h in large:
            a, b = row[h], col[h]
            o["inter"] += 1
            o["w_row"] += a
            o["w_col"] += b
            o["w_min"] += min(a, b)
            o["dot_lo"] += (a * b) & MASK32
            o["dot_hi"] += (a * b) >> 32
    return o


def dot(o):
    return (o["dot_hi"] << 32) + o["dot_lo"]


def totals(s):
    """-> (S, Q_lo, Q_hi) of a sample"""
    return (sum(s.values()), sum((a * a) & MASK32 for a in s.values()), sum((a * a) >> 32 for a in s.values()))


def _div(num, den):
    """fp64 num / den with IEEE results where Python raises"""
    if den == 0.0:
        return math.nan if num == 0.0 or num != num else math.copysign(math.inf, num)
    return num / den


def similarity(o, t_row, t_col):
    """mvs_abund_similarity: o = the six fields, t_* = (S, Q_lo, Q_hi) -> dict of the six measures"""
    s_row, s_col = t_row[0], t_col[0]
    q_row, q_col = (t_row[2] << 32) + t_row[1], (t_col[2] << 32) + t_col[1]
    both = s_row + s_col
    m = {}
    m["w_contain_row"] = _div(float(o["w_row"]), float(s_row))
    m["w_contain_col"] = _div(float(o["w_col"]), float(s_col))
    m["bray_curtis"] = _div(float(both - 2 * o["w_min"]), float(both))
    m["ruzicka"] = _div(float(o["w_min"]), float(both - o["w_min"]))
    product = float(q_row) * float(q_col)
    cosine = _div(float(dot(o)), math.sqrt(product))
    if cosine > 1.0:
        cosine = 1.0
    m["cosine"] = cosine
    m["angular"] = math.nan if cosine != cosine else 1.0 - 2.0 * math.acos(cosine) / math.pi
    return m


def cell(row, col):
    """-> (fields, measures) of one cell"""
    o = overlap(row, col)
    return o, similarity(o, totals(row), totals(col))
