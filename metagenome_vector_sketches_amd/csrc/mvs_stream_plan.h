// mvs_stream_plan.h -- the arithmetic of the streamed output (mvs_capi_stream.hip): how a row range is cut into row blocks,
// which blocks open a filter segment, how a block is cut into pieces for the link, and the estimates that choose a route.
// Host-only and free of the runtime: host/mvs_stream_plan_selftest.cpp pins every function without a device.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace mvs_capi {

inline int bits_for(int64_t max_value) {   // bits that hold 0 .. max_value
    int b = 1;
    while (b < 63 && (max_value >> b) != 0) ++b;
    return b;
}

// ---- pieces: a block leaves through the pinned buffers in runs of whole rows ----
// offsets[0 .. rows] are running totals (cells or bytes).  The piece that starts at row r0 ends at the returned row: as many
// whole rows as fit `limit`; one row alone may exceed it.
template <typename T>
int64_t piece_end(const T* offsets, int64_t rows, int64_t r0, T limit) {
    int64_t r1 = r0 + 1;
    const T o0 = offsets[r0];
    if (offsets[r1] - o0 <= limit) {
        const T* end = std::upper_bound(offsets + r1, offsets + rows + 1, o0 + limit);
        r1 = std::max<int64_t>(r1, (end - offsets) - 1);
    }
    return r1;
}
// ... and the largest piece of the block, in the offsets' unit (sizes a pinned buffer)
template <typename T>
T largest_piece(const T* offsets, int64_t rows, T limit) {
    T most = 0;
    for (int64_t r0 = 0; r0 < rows;) {
        const int64_t r1 = piece_end(offsets, rows, r0, limit);
        most = std::max<T>(most, offsets[r1] - offsets[r0]);
        r0 = r1;
    }
    return most;
}

// ---- row blocks ----
// rows of a packed-list block: its worst case -- every cell kept -- fits budget_cells, and the row field fits the packed word
// above `shift` bits of (column, q)
inline int64_t list_block_rows(int64_t budget_cells, int64_t n, int shift) {
    int64_t br = std::max<int64_t>(256, budget_cells / std::max<int64_t>(n, 1) / 256 * 256);
    while (shift + bits_for(std::max<int64_t>(br - 1, 1)) > 64 && br > 256) br /= 2;
    return br;
}

// rows of a dense-matrix block; 0 = not even 256 rows of bytes fit: list blocks instead.  whole: the blocks share one matrix
// of all the rows; otherwise the matrix holds one block (budget / ld rows).  stream_block_rows > 0 (tests): an upper bound.
inline int64_t dense_block_rows(bool whole, int64_t rows_all, size_t dense_budget, int64_t ld, int64_t stream_block_rows) {
    int64_t block_rows;
    if (whole) {
        block_rows = std::max<int64_t>(2048, (rows_all / 16 + 255) / 256 * 256);   // (1/12 .. 1/6 of the rows measure the same or worse)
    } else {
        block_rows = (int64_t)(dense_budget / (size_t)ld) / 256 * 256;
        if (block_rows < 256) return 0;
    }
    if (stream_block_rows > 0)                                  // tests: many small blocks on small inputs
        block_rows = std::min<int64_t>(block_rows, std::max<int64_t>(256, stream_block_rows / 256 * 256));
    return block_rows;
}

typedef std::vector<std::pair<int64_t, int64_t>> RowBlocks;

// [row_begin, row_end) in blocks that end on 256-row borders: the first holds first_ramp rows, each next one twice the one
// before, up to block_rows
inline RowBlocks row_blocks(int64_t row_begin, int64_t row_end, int64_t block_rows, int64_t first_ramp) {
    RowBlocks blocks;
    int64_t ramp = first_ramp;
    for (int64_t rb = row_begin; rb < row_end;) {
        const int64_t re = std::min(row_end, (rb / 256) * 256 + std::min(ramp, block_rows));
        blocks.emplace_back(rb, re);
        rb = re;
        ramp = std::min(block_rows, ramp * 2);
    }
    return blocks;
}

// M1: which blocks open a filter segment.  Segment 0 is the probe (one tile row); the others end where 4 %, 16 % and 45 %
// of the rows are done -- by the tiles of the symmetric square that is 8 %, 22 %, 40 % and 30 % of the filter's work --
// every_block (option stream_block_rows, tests) makes every block a segment of its own.
inline std::vector<char> segment_opens(const RowBlocks& blocks, int64_t row_begin, int64_t row_end, bool every_block) {
    std::vector<char> seg_first(blocks.size(), 0);
    const double marks[3] = {0.04, 0.16, 0.45};   // (0.05 / 0.3, 0.03 / 0.12 / 0.3, 0.1 / 0.4 measure the same within 2 %)
    int next_mark = 0;
    for (size_t k = 0; k < blocks.size(); ++k) {
        const double done = (double)(blocks[k].first - row_begin) / (double)(row_end - row_begin);
        bool opens = k <= 1 || every_block;
        while (next_mark < 3 && done >= marks[next_mark]) {
            opens = true;
            ++next_mark;
        }
        seg_first[k] = opens ? 1 : 0;
    }
    return seg_first;
}

// ---- route estimates ----
// M1's probe: the share of flagged tiles in one row of tiles, extrapolated to the tiles of the whole pass, as list cells
inline double probe_list_cells(int n_flagged, unsigned long long n_cand, int n_tr_all, int n_tc_all) {
    const double tiles_all = std::max(1.0, (double)n_tr_all * (double)n_tc_all - 0.5 * (double)n_tr_all * (double)(n_tr_all - 1));
    return ((double)n_flagged * 131072.0 + 2.0 * (double)n_cand) / (double)n_tc_all * tiles_all;
}
// plan A: an upper bound on the kept cells of a whole filter pass (a kept cell is a candidate or the mirror image of one, or a
// cell of a flagged 256 x 256 tile or of its mirror image)
inline unsigned long long list_bound(unsigned long long n_cand, int n_flagged) {
    return 2 * n_cand + (unsigned long long)n_flagged * 131072ULL;
}

}  // namespace mvs_capi
