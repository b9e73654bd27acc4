// mvs_stream_plan_selftest.cpp -- the arithmetic of the streamed output (../mvs_stream_plan.h) against values written out by
// hand: row blocks with their doubling ramp and 256-row borders, the blocks that open a filter segment, block sizes for lists
// and for the dense matrix, pieces of whole rows under a limit, the route estimates.  No device and no HIP library; `make
// asan` builds it again with the sanitizers.
#include <cstdio>
#include <string>

#include "../mvs_stream_plan.h"

using namespace mvs_capi;

static int g_bad = 0;
static void check(bool ok, const char* what, int line) {
    if (!ok) {
        std::printf("FAILED line %d: %s\n", line, what);
        ++g_bad;
    }
}
#define CHECK(x) check((x), #x, __LINE__)

static std::string show(const RowBlocks& blocks) {
    std::string s;
    for (const auto& b : blocks) s += "[" + std::to_string(b.first) + "," + std::to_string(b.second) + ") ";
    return s;
}
static std::string show(const std::vector<char>& flags) {
    std::string s;
    for (char f : flags) s += f ? "1 " : "0 ";
    return s;
}
// every piece of a block, and the largest
template <typename T>
static std::string pieces(const std::vector<T>& off, T limit, T* largest) {
    const int64_t rows = (int64_t)off.size() - 1;
    RowBlocks p;
    for (int64_t r0 = 0; r0 < rows;) {
        const int64_t r1 = piece_end(off.data(), rows, r0, limit);
        CHECK(r1 > r0 && r1 <= rows);
        p.emplace_back(r0, r1);
        r0 = r1;
    }
    *largest = largest_piece(off.data(), rows, limit);
    return show(p);
}

int main() {
    CHECK(bits_for(0) == 1 && bits_for(1) == 1 && bits_for(2) == 2 && bits_for(255) == 8 && bits_for(256) == 9);
    CHECK(bits_for(16383) == 14 && bits_for(INT64_MAX) == 63);

    // ---- row blocks ----
    CHECK(show(row_blocks(0, 5000, 2048, 1024)) == "[0,1024) [1024,3072) [3072,5000) ");
    const RowBlocks twelve = row_blocks(0, 20000, 2048, 256);
    CHECK(show(twelve) ==
          "[0,256) [256,768) [768,1792) [1792,3840) [3840,5888) [5888,7936) [7936,9984) [9984,12032) [12032,14080) [14080,16128) "
          "[16128,18176) [18176,20000) ");
    CHECK(twelve.size() == 12);
    CHECK(show(segment_opens(twelve, 0, 20000, false)) == "1 1 0 1 1 0 0 1 0 0 0 0 ");
    CHECK(show(segment_opens(twelve, 0, 20000, true)) == "1 1 1 1 1 1 1 1 1 1 1 1 ");
    const RowBlocks four = row_blocks(512, 3000, 2048, 256);
    CHECK(show(four) == "[512,768) [768,1280) [1280,2304) [2304,3000) ");
    CHECK(show(segment_opens(four, 512, 3000, false)) == "1 1 1 1 ");      // (the marks are crossed at k = 2 and k = 3)
    CHECK(show(row_blocks(100, 1000, 256, 256)) == "[100,256) [256,512) [512,768) [768,1000) ");      // unaligned start
    CHECK(show(row_blocks(300, 1500, 512, 512)) == "[300,768) [768,1280) [1280,1500) ");
    CHECK(row_blocks(7, 7, 256, 256).empty());

    // ---- block sizes ----
    CHECK(list_block_rows(1 << 20, 4096, 16 + 12) == 256);                 // what the budget gives
    CHECK(list_block_rows(3000000, 1000, 16 + 10) == 2816);                // ... rounded down to whole tiles
    CHECK(list_block_rows(1000, 4096, 16 + 12) == 256);                    // ... never below one tile row
    CHECK(list_block_rows(1LL << 30, 1024, 50) == 16384);                  // 2^20 rows would need 20 bits above 50: halved to 14
    CHECK(dense_block_rows(true, 100000, 0, 100096, 0) == 6400);           // shared matrix: a sixteenth of the rows
    CHECK(dense_block_rows(true, 5000, 0, 5120, 0) == 2048);               // ... at least 2048
    CHECK(dense_block_rows(false, 100000, (size_t)600 * 100096, 100096, 0) == 512);      // a matrix per block: what the budget holds
    CHECK(dense_block_rows(false, 100000, (size_t)200 * 100096, 100096, 0) == 0);        // not even a tile row: lists
    CHECK(dense_block_rows(true, 100000, 0, 100096, 200) == 256);          // stream_block_rows clamps, to a tile row at least
    CHECK(dense_block_rows(true, 100000, 0, 100096, 1000) == 768);
    CHECK(dense_block_rows(false, 100000, (size_t)200 * 100096, 100096, 200) == 0);      // (no clamp turns "lists" into a block)

    // ---- pieces ----
    int64_t most = 0;
    CHECK(pieces<int64_t>({0, 3, 3, 10, 11}, 4, &most) == "[0,2) [2,3) [3,4) " && most == 7);     // a row of 7 alone exceeds the limit
    CHECK(pieces<int64_t>({0, 0, 4, 8, 8, 9}, 4, &most) == "[0,2) [2,4) [4,5) " && most == 4);
    CHECK(pieces<int64_t>({0, 5}, 4, &most) == "[0,1) " && most == 5);
    CHECK(pieces<int64_t>({0, 0, 0}, 4, &most) == "[0,2) " && most == 0);                         // only empty rows
    uint64_t most_u = 0;                                                                          // ... and on byte offsets
    CHECK(pieces<uint64_t>({0, 3, 3, 10, 11}, 4, &most_u) == "[0,2) [2,3) [3,4) " && most_u == 7);
    CHECK(pieces<uint64_t>({0, 0, 4, 8, 8, 9}, 4, &most_u) == "[0,2) [2,4) [4,5) " && most_u == 4);

    // ---- route estimates ----
    // 40 x 40 tiles, symmetric: 1600 - 780 = 820 tiles in the pass; (10 * 131072 + 2 * 1000) / 40 per tile of the probe's row
    CHECK(probe_list_cells(10, 1000, 40, 40) == 26910760.0);
    CHECK(probe_list_cells(0, 0, 1, 1) == 0.0);
    CHECK(list_bound(1000, 10) == 1312720ULL);
    CHECK(list_bound(3000000000ULL, 0) == 6000000000ULL);                  // (64-bit: beyond 2^32)

    if (g_bad) {
        std::printf("%d check(s) FAILED\n", g_bad);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
