// mvs_project.hip -- projection kernels (gfx950 / CDNA4).
//
// Reference semantics: transform_set_into_vector(), src/random_projection.cpp:9-26
//   v[k] = sum_h (1 - 2*bit_{k%64}(SM(h + 64*(k/64))))  ==  n - 2*count_k
// where count_k = number of hashes whose bit k%64 of SM(h + 64*(k/64)) is set.
//
// MI355X design (see DESIGN.md "K1"):
//   * the +-1 matrix is implicit (hash generated), so there is nothing to stage from HBM; the kernel
//     is integer-VALU bound (19 VALU per splitmix64 on its own, 6 of them 32-bit multiplies; the last xorshift's
//     two xors are not among the kernel's: they happen inside the counters' first adder, see absorb);
//   * the instructions are not equally expensive: xor, two-operand add and bitop3 issue in 2.7-2.8 cycles, every multiply,
//     shift and three-operand add in 4.2-4.65.  Each 64-bit multiply of the hash is v_mad_u64_u32(lo, C.lo, {0, cross
//     terms}) (mad64): the addend of the mad, which is free, carries what a v_add3_u32 added behind it, and a v_add_u32
//     is what is left.  Same count, cheaper mix (tools/check_project_isa.py prices it);
//   * each LANE hashes its own stream of hashes (coalesced 8-byte loads, 512 B per wave load) and
//     counts set bits per position with BIT-SLICED counters: a Harley-Seal carry-save tree built from
//     v_bitop3_b32 full adders (xor3 / majority), ~4.6 VALU per (hash, 64-dim block) instead of 128
//     extract+add; the level-1 adder takes the hash as (w, w >> 31) and needs 3 bitop3 per two leaf words where
//     2 xors + 2 bitop3 were 4.  Hot loop of the default variant (24): 19.38 VALU per (hash, block)
//     (tools/check_project_isa.py);
//   * one wave owns BPW 64-dim blocks of one (sample, hash-chunk) unit; at the end the 64 lanes'
//     bit-sliced counters are summed by a butterfly of bit-sliced ripple adders.  The default variant (24) does it
//     inside the VALU (v_permlane*_swap and DPP moves, no LDS) and for its four blocks together: the stages hand
//     different lanes different blocks, a lane ends with the total of one block's half, extracts four consecutive
//     counts and writes them with one 16-byte store (reduce_counts_wave4: 10 LV0 + 16 digit additions per wave where
//     an all-reduce per block did 24 LV0 + 60).  The other variants reduce block by block through ds_bpermute and
//     lane k extracts count_k (reduce_counts);
//   * samples are cut into units of <= 65536 hashes so that long samples spread over many
//     workgroups, and the units that would run past the launch's ideal end into smaller pieces
//     (mvs_project_plan); units of one sample combine with int32 atomics (order independent => exact).
#include "mvs_internal.h"

namespace mvs {

namespace {

constexpr int kLV = 11;            // bit-sliced counter depth per lane: counts up to 2047
constexpr uint64_t kGolden = 0x9e3779b97f4a7c15ULL;

// truth table of a three-input boolean function as v_bitop3_b32 wants it: bit (src0 << 2 | src1 << 1 | src2) of the
// constant is f(src0, src1, src2)
template <class F>
constexpr uint32_t bitop3_table(F f) {
    uint32_t t = 0;
    for (uint32_t i = 0; i < 8; ++i)
        if (f((i >> 2) & 1u, (i >> 1) & 1u, i & 1u) & 1u) t |= 1u << i;
    return t;
}
constexpr uint32_t bit_xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
constexpr uint32_t bit_maj3(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (a & c) | (b & c); }
// the carry of s + a + b from s, u = s ^ a and m = s ^ a ^ b (the two running sums a level-1 adder forms anyway):
// a = s ^ u and b = u ^ m.  Not symmetric in its operands.
constexpr uint32_t bit_carry_sum(uint32_t s, uint32_t u, uint32_t m) { return bit_maj3(s, s ^ u, u ^ m); }
constexpr uint32_t kXor3 = bitop3_table(bit_xor3), kMaj3 = bitop3_table(bit_maj3), kCarrySum = bitop3_table(bit_carry_sum);
static_assert(kXor3 == 0x96 && kMaj3 == 0xE8, "operand order of the bitop3 truth table");

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, kXor3);
}
__device__ __forceinline__ uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, kMaj3);
}
__device__ __forceinline__ uint32_t carry_sum(uint32_t s, uint32_t u, uint32_t m) {
    return __builtin_amdgcn_bitop3_b32(s, u, m, kCarrySum);
}

// v >> N as ONE v_lshrrev_b64.  Where only the halves of the result are used, the compiler splits a plain 64-bit shift
// into v_alignbit_b32 + v_lshrrev_b32, two instructions of the same issue class as the one.  Not volatile: it schedules
// like any other instruction.
template <int N>
__device__ __forceinline__ uint64_t shr64(uint64_t v) {
    static_assert(N > 0 && N < 64, "shift count");
    uint64_t r;
    asm("v_lshrrev_b64 %0, %1, %2" : "=v"(r) : "n"(N), "v"(v));
    return r;
}

constexpr uint32_t kC1Lo = 0x1ce4e5b9u, kC1Hi = 0xbf58476du;
constexpr uint32_t kC2Lo = 0x133111ebu, kC2Hi = 0x94d049bbu;

// a * b + c as ONE v_mad_u64_u32 whose 64-bit addend does work: a 64-bit multiply by a constant C is
//     lo * C.lo + ((lo * C.hi + hi * C.lo) << 32)   (mod 2^64),
// and with the cross terms in the addend's high half the sum behind the multiply is a two-operand v_add_u32 (or nothing)
// where a zero addend leaves a v_add3_u32, an instruction of the multiplies' issue class.  Inline asm because the compiler
// will not form it: it splits c off again (v_mul_lo_u32 + adds) or wraps the mad in moves to align its register pairs.
// b is a constant in an SGPR; the carry out goes to an SGPR pair nobody reads.
__device__ __forceinline__ uint64_t mad64(uint32_t a, uint32_t b, uint64_t c) {
    uint64_t r, carry;
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(carry) : "v"(a), "s"(b), "v"(c));
    return r;
}
// a * b with the multiply hidden from the compiler, which would fold it and the add behind it into a v_mad_u64_u32 of its
// own, with a 32-bit addend widened by two moves
__device__ __forceinline__ uint32_t mul_lo(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_mul_lo_u32 %0, %1, %2" : "=v"(r) : "v"(a), "s"(b));
    return r;
}

// z * C for a constant C = {clo, chi}, cross terms in the mad's addend; zero is a register that holds 0 (see k_project)
__device__ __forceinline__ uint64_t mul64_mad(uint64_t z, uint32_t clo, uint32_t chi, uint32_t zero) {
    const uint32_t zl = (uint32_t)z, zh = (uint32_t)(z >> 32);
    const uint32_t cross = mul_lo(zl, chi) + mul_lo(zh, clo);
    return mad64(zl, clo, ((uint64_t)cross << 32) | (uint64_t)zero);
}

// src/random_projection.cpp:14-16 applied to z = hash + i + 0x9e37... (the adds of :13-14 are folded
// into one 64-bit add by the caller): splitmix64 up to its second multiply.  MAD: both multiplies as mul64_mad.
template <bool MAD>
__device__ __forceinline__ uint64_t splitmix_mul2(uint64_t z, uint32_t zero) {
    if constexpr (MAD) {
        z = mul64_mad(z ^ (z >> 30), kC1Lo, kC1Hi, zero);
        return mul64_mad(z ^ (z >> 27), kC2Lo, kC2Hi, zero);
    } else {
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        return (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    }
}
// ... and :17, the last xorshift
template <bool MAD>
__device__ __forceinline__ uint64_t splitmix_tail(uint64_t z, uint32_t zero) {
    z = splitmix_mul2<MAD>(z, zero);
    return z ^ (z >> 31);
}

template <int BPW>
struct Acc {
    uint32_t lo[BPW][kLV];
    uint32_t hi[BPW][kLV];
};

// Harley-Seal: absorb 2^LEVEL inputs into the persistent bit-sliced digits s[0..LEVEL-1]; returns
// (in clo/chi) the carry word of weight 2^LEVEL.  2^LEVEL - 1 full adders per 2^LEVEL inputs.
//
// The level-1 adder takes its two leaves unfinished: a leaf is w ^ t with t = w >> 31 (the last xorshift of splitmix64),
// and nothing else ever reads it, so the xor happens inside the adder.  With u = s ^ a and m = s ^ a ^ b
//     u = xor3(s, wa, ta),   m = xor3(u, wb, tb) (the new digit),   carry = maj(s, a, b) = carry_sum(s, u, m)
// are three bitop3 per word where xor, xor, xor3, maj3 were four.  Leaf A is produced and folded into u for every block
// before leaf B is produced: with both leaves' (w, t) alive at once the BPW = 4 kernels do not fit two waves per SIMD.
template <int LEVEL, int BPW, class Gen>
__device__ __forceinline__ void absorb(Acc<BPW>& s, Gen& g, uint32_t (&clo)[BPW], uint32_t (&chi)[BPW]) {
    if constexpr (LEVEL == 0) {
        g.next(clo, chi);
    } else if constexpr (LEVEL == 1) {
        uint32_t wl[BPW], wh[BPW], tl[BPW], th[BPW], ul[BPW], uh[BPW];
        g.next_unmixed(wl, wh, tl, th);
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            ul[b] = xor3(s.lo[b][0], wl[b], tl[b]);
            uh[b] = xor3(s.hi[b][0], wh[b], th[b]);
        }
        g.next_unmixed(wl, wh, tl, th);
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            const uint32_t ml = xor3(ul[b], wl[b], tl[b]), mh = xor3(uh[b], wh[b], th[b]);
            clo[b] = carry_sum(s.lo[b][0], ul[b], ml);
            chi[b] = carry_sum(s.hi[b][0], uh[b], mh);
            s.lo[b][0] = ml;
            s.hi[b][0] = mh;
        }
    } else {
        uint32_t alo[BPW], ahi[BPW], blo[BPW], bhi[BPW];
        absorb<LEVEL - 1, BPW>(s, g, alo, ahi);
        absorb<LEVEL - 1, BPW>(s, g, blo, bhi);
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            const uint32_t tl = s.lo[b][LEVEL - 1], th = s.hi[b][LEVEL - 1];
            clo[b] = maj3(tl, alo[b], blo[b]);
            chi[b] = maj3(th, ahi[b], bhi[b]);
            s.lo[b][LEVEL - 1] = xor3(tl, alo[b], blo[b]);
            s.hi[b][LEVEL - 1] = xor3(th, ahi[b], bhi[b]);
        }
    }
}

// add a carry word of weight 2^FROM into digits FROM..kLV-1 (half adders)
template <int FROM, int BPW>
__device__ __forceinline__ void ripple(Acc<BPW>& s, uint32_t (&clo)[BPW], uint32_t (&chi)[BPW]) {
#pragma unroll
    for (int l = FROM; l < kLV; ++l) {
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            const uint32_t tl = s.lo[b][l] & clo[b], th = s.hi[b][l] & chi[b];
            s.lo[b][l] ^= clo[b];
            s.hi[b][l] ^= chi[b];
            clo[b] = tl;
            chi[b] = th;
        }
    }
}

// yields SM(h + 64*block) for the next hash of a register-resident batch, for each of the wave's BPW
// blocks.  The batch (8 hashes per lane = 512 per wave) was loaded one batch ahead of its use.
template <int BPW, bool MASKED, bool MAD>
struct BatchGen {
    const uint64_t (&h)[8];
    const uint64_t (&cb)[BPW];   // 64*block + golden
    const uint32_t (&zero)[BPW]; // MAD: registers that hold 0
    int64_t remaining;           // MASKED: hashes left from this lane's first hash of the batch
    int j = 0;
    __device__ __forceinline__ BatchGen(const uint64_t (&h_)[8], const uint64_t (&cb_)[BPW], const uint32_t (&zero_)[BPW], int64_t rem)
        : h(h_), cb(cb_), zero(zero_), remaining(rem) {}
    __device__ __forceinline__ void next(uint32_t (&lo)[BPW], uint32_t (&hi)[BPW]) {
        const uint64_t hv = h[j];
        bool valid = true;
        if constexpr (MASKED) valid = (int64_t)j * 64 < remaining;
        ++j;
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            uint64_t x = splitmix_tail<MAD>(hv + cb[b], zero[b]);
            if constexpr (MASKED) x = valid ? x : 0ULL;
            lo[b] = (uint32_t)x;
            hi[b] = (uint32_t)(x >> 32);
        }
    }
    // the same hash without its last xorshift, for the level-1 adder: w after the second multiply and t = w >> 31
    // (leaf = w ^ t); an invalid slot yields four zero words
    __device__ __forceinline__ void next_unmixed(uint32_t (&wl)[BPW], uint32_t (&wh)[BPW], uint32_t (&tl)[BPW],
                                                 uint32_t (&th)[BPW]) {
        const uint64_t hv = h[j];
        bool valid = true;
        if constexpr (MASKED) valid = (int64_t)j * 64 < remaining;
        ++j;
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            uint64_t w = splitmix_mul2<MAD>(hv + cb[b], zero[b]);
            if constexpr (MASKED) w = valid ? w : 0ULL;
            const uint64_t t = shr64<31>(w);
            wl[b] = (uint32_t)w;
            wh[b] = (uint32_t)(w >> 32);
            tl[b] = (uint32_t)t;
            th[b] = (uint32_t)(t >> 32);
        }
    }
};

// The same values for a wave that owns BPW CONSECUTIVE blocks, with the part of the first splitmix64 round that the
// blocks share computed once per hash.  x_b = x_0 + 64 b differs from x_0 only below bit 30 unless the addition carries
// out of bit 29; without that carry  x_b >> 30 == x_0 >> 30 =: t  and the high word of x_b equals that of x_0, so
//     z_b = x_b ^ (x_b >> 30)  has  z_b.hi = x_0.hi ^ t.hi  (shared)  and  z_b.lo = (x_0.lo + 64 b) ^ t.lo ,
//     z_b * C1 mod 2^64 = z_b.lo * C1.lo  +  ((z_b.lo * C1.hi + z_b.hi * C1.lo) << 32)     with z_b.hi * C1.lo shared.
// Per block that saves the 64-bit add, the 64-bit shift, one xor and one of the four 32-bit multiplies of the round
// (9 quarter-rate instructions per hash at BPW = 4).  The carry case -- bits 8..29 of x_0 all ones, one hash in 4 million
// -- is detected per batch by hazard() and such a batch goes through BatchGen (the wave-uniform branch costs nothing
// when it is not taken), so every value is exact.
// ROUND2: the second multiply the same way.  Its addend is {0, cross}, and the zero low half has to cost nothing: zero[b] is a
// register the kernel writes once (opaque to the compiler, which would otherwise write a fresh zero per multiply), one per
// block so that consecutive blocks' addends can be alive together.
template <int BPW, bool ROUND2>
struct BatchGenShared {
    const uint64_t (&x)[8];      // hash + 64 * first block + golden (the sums hazard() has looked at)
    const uint32_t (&zero)[BPW];
    int j = 0;
    __device__ __forceinline__ BatchGenShared(const uint64_t (&x_)[8], const uint32_t (&zero_)[BPW]) : x(x_), zero(zero_) {}
    // without the last xorshift, for the level-1 adder: (w, t = w >> 31) with w the value after the second multiply,
    // leaf = w ^ t.  The only producer: this generator feeds whole batches (absorb<3>), never a lone leaf.
    __device__ __forceinline__ void next_unmixed(uint32_t (&wl)[BPW], uint32_t (&wh)[BPW], uint32_t (&tl)[BPW],
                                                 uint32_t (&th)[BPW]) {
        const uint64_t x0 = x[j++];
        const uint64_t t0 = shr64<30>(x0);
        const uint32_t x0l = (uint32_t)x0, t0l = (uint32_t)t0;
        const uint32_t zh = (uint32_t)(x0 >> 32) ^ (uint32_t)(t0 >> 32);
        const uint64_t p64 = (uint64_t)(zh * kC1Lo) << 32;       // the shared cross term, where the mad adds it
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            const uint32_t zl = (x0l + 64u * (uint32_t)b) ^ t0l;
            const uint64_t m = mad64(zl, kC1Lo, p64);
            const uint32_t whi = (uint32_t)(m >> 32) + mul_lo(zl, kC1Hi);
            const uint64_t v = ((uint64_t)whi << 32) | (uint64_t)(uint32_t)m;
            const uint64_t u = v ^ (v >> 27);
            uint64_t w;
            if constexpr (ROUND2) {
                const uint32_t ul = (uint32_t)u, uh = (uint32_t)(u >> 32);
                const uint32_t cross = mul_lo(ul, kC2Hi) + mul_lo(uh, kC2Lo);
                w = mad64(ul, kC2Lo, ((uint64_t)cross << 32) | (uint64_t)zero[b]);
            } else {
                w = u * 0x94d049bb133111ebULL;
            }
            const uint64_t t = shr64<31>(w);
            wl[b] = (uint32_t)w;
            wh[b] = (uint32_t)(w >> 32);
            tl[b] = (uint32_t)t;
            th[b] = (uint32_t)(t >> 32);
        }
    }
};

// x[j] = h[j] + cb0 for the batch; true if some hash of it could carry out of bit 29 when 64 * b (b < 4) is added
__device__ __forceinline__ bool hazard(const uint64_t (&h)[8], uint64_t cb0, uint64_t (&x)[8]) {
    uint32_t least = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        x[j] = h[j] + cb0;
        const uint32_t xl = (uint32_t)x[j];
        const uint32_t miss = ~xl & 0x3fffff00u;                 // zero <=> bits 8..29 are all ones
        least = miss < least ? miss : least;
    }
    return __any(least == 0u) != 0;
}

// load the batch that starts at hash index `pos` of the unit; indices are clamped into the unit so the
// prefetch of a batch that does not exist (or the tail of a partial one) stays in bounds
template <bool CLAMP>
__device__ __forceinline__ void load_batch(uint64_t (&h)[8], const uint64_t* base, int64_t pos, int lane,
                                           int64_t last) {
    if constexpr (CLAMP) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int64_t idx = pos + j * 64 + lane;
            idx = idx < last ? idx : last;
            h[j] = base[idx];
        }
    } else {
        const uint64_t* p = base + pos + lane;   // whole batch known to be inside the unit
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = p[j * 64];
    }
}

// Sum the 64 lanes' bit-sliced counters and return, in lane k, the count for bit position k.  LV0 = number of
// counter digits that can be non-zero (every lane absorbed fewer than 2^LV0 hashes): short units skip the dead
// digits, which is most of this step's work (6*LV0 + 21 digit additions).
template <int LV0>
__device__ __forceinline__ int32_t reduce_counts(const uint32_t (&lo_in)[kLV], const uint32_t (&hi_in)[kLV],
                                                 int lane) {
    static_assert(LV0 >= 1 && LV0 <= kLV, "live digits");
    constexpr int kOut = LV0 + 6;
    uint32_t lo[kOut], hi[kOut];
#pragma unroll
    for (int l = 0; l < kOut; ++l) {
        lo[l] = l < LV0 ? lo_in[l] : 0u;
        hi[l] = l < LV0 ? hi_in[l] : 0u;
    }
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        uint32_t cl = 0, ch = 0;
#pragma unroll
        for (int l = 0; l < LV0 + s + 1; ++l) {
            const uint32_t pl = (uint32_t)__shfl_xor((int)lo[l], 1 << s, 64);
            const uint32_t ph = (uint32_t)__shfl_xor((int)hi[l], 1 << s, 64);
            const uint32_t sl = xor3(lo[l], pl, cl), sh = xor3(hi[l], ph, ch);
            cl = maj3(lo[l], pl, cl);
            ch = maj3(hi[l], ph, ch);
            lo[l] = sl;
            hi[l] = sh;
        }
    }
    int32_t cnt = 0;
    const int sh = lane & 31;
#pragma unroll
    for (int l = 0; l < kOut; ++l) {
        const uint32_t w = lane < 32 ? lo[l] : hi[l];
        cnt += (int32_t)((w >> sh) & 1u) << l;
    }
    return cnt;
}

// The same sums without LDS (DEEP): every cross-lane move is a DPP move or a v_permlane*_swap, all inside the VALU.  A lane
// only needs the digits of one word (lo: positions 0-31, hi: 32-63), so the first step adds the two 32-lane halves AND
// merges lo with hi: v_permlane32_swap(lo, hi) hands lanes 0-31 the pair (lo[k], lo[k + 32]) and lanes 32-63 the pair
// (hi[k - 32], hi[k]).  From there on one word per digit is reduced instead of two.  A swap leaves {own, partner} in its two
// outputs in some order, and the sum of the two is the same either way.
__device__ __forceinline__ void add_digit(uint32_t& w, uint32_t a, uint32_t b, uint32_t& c) {
    w = xor3(a, b, c);
    c = maj3(a, b, c);
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}

// one stage on the LIVE low digits of w; the carry out becomes digit LIVE
template <int CTRL, int LIVE, int N>
__device__ __forceinline__ void reduce_stage_dpp(uint32_t (&w)[N]) {
    static_assert(LIVE < N, "room for the carry");
    uint32_t c = 0;
#pragma unroll
    for (int l = 0; l < LIVE; ++l) {
        add_digit(w[l], w[l], dpp_mov<CTRL>(w[l]), c);
    }
    w[LIVE] = c;
}

// The four blocks of a BPW = 4 wave reduced TOGETHER.  An all-reduce per block (five more stages over the 32 lanes of a
// half behind the first) leaves all 32 lanes of a half with the same total, of which each extracts one position: (LV0 + 1)
// + ... + (LV0 + 5) additions behind the first LV0, per block.  Here every stage that can hands different lanes
// different blocks, so the words halve as the lanes to add do, and a lane ends with the total of ONE block's half and
// extracts four positions of it:
//   stage 0  per block as above: v_permlane32_swap(lo, hi), lanes 0-31 hold the lo word (positions 0-31), 32-63 the hi word;
//   stage 1  v_permlane16_swap(W_a, W_b) exchanges rows 1, 3 of W_a with rows 0, 2 of W_b: the sum of its two outputs is
//            block a over both rows of the half in rows 0, 2 and block b in rows 1, 3.  One addition serves two blocks
//            (a, b) = (0, 1) -> X and (2, 3) -> Y;
//   stage 2  lanes i and i ^ 1: even lanes keep X and get the neighbour's X, odd lanes keep Y and get the neighbour's Y
//            (two selects, one DPP move);
//   stages 3-5  all-reduce over the 8 lanes of a row with the same parity: quad_perm [2,3,0,1], row_ror:4, row_ror:8.
// Row r = lane >> 4 then holds half r >> 1 of block (r & 1) + 2 * (lane & 1), and lane j = (lane & 15) >> 1 of the eight
// holders extracts positions 4j .. 4j + 3 of that half into cnt.  Digit additions: 4 LV0 + 2 (LV0 + 1) + (LV0 + 2) + ... +
// (LV0 + 5) = 10 LV0 + 16 where four all-reduces do 24 LV0 + 60.
//
// The extraction takes the lane's four bits of a digit at once: n * 0x00204081 spreads the nibble n over the low bits of
// four bytes (n, n << 7, n << 14, n << 21 do not overlap), and with the digit's shift inside the constant three
// instructions per digit (bfe, mul, and_or) build byte-packed counts, eight digits per accumulator.
template <int LV0>
__device__ __forceinline__ void reduce_pair_stage01(const uint32_t (&lo_a)[kLV], const uint32_t (&hi_a)[kLV],
                                                    const uint32_t (&lo_b)[kLV], const uint32_t (&hi_b)[kLV],
                                                    uint32_t (&x)[LV0 + 6]) {
    uint32_t wa[LV0 + 1], wb[LV0 + 1];
    uint32_t ca = 0, cb = 0;
#pragma unroll
    for (int l = 0; l < LV0; ++l) {
        const auto ra = __builtin_amdgcn_permlane32_swap(lo_a[l], hi_a[l], false, false);
        add_digit(wa[l], ra[0], ra[1], ca);
        const auto rb = __builtin_amdgcn_permlane32_swap(lo_b[l], hi_b[l], false, false);
        add_digit(wb[l], rb[0], rb[1], cb);
    }
    wa[LV0] = ca;
    wb[LV0] = cb;
    uint32_t c = 0;
#pragma unroll
    for (int l = 0; l < LV0 + 1; ++l) {
        const auto r = __builtin_amdgcn_permlane16_swap(wa[l], wb[l], false, false);
        add_digit(x[l], r[0], r[1], c);
    }
    x[LV0 + 1] = c;
}

template <int LV0>
__device__ __forceinline__ void reduce_counts_wave4(const Acc<4>& s, int lane, int32_t (&cnt)[4]) {
    static_assert(LV0 >= 1 && LV0 <= kLV, "live digits");
    constexpr int kOut = LV0 + 6;
    uint32_t x[kOut], y[kOut];
    reduce_pair_stage01<LV0>(s.lo[0], s.hi[0], s.lo[1], s.hi[1], x);
    reduce_pair_stage01<LV0>(s.lo[2], s.hi[2], s.lo[3], s.hi[3], y);
    const bool odd = (lane & 1) != 0;
    uint32_t c = 0;
#pragma unroll
    for (int l = 0; l < LV0 + 2; ++l) {
        const uint32_t send = odd ? x[l] : y[l], keep = odd ? y[l] : x[l];
        add_digit(x[l], keep, dpp_mov<0xb1>(send), c);   // quad_perm [1,0,3,2]
    }
    x[LV0 + 2] = c;
    reduce_stage_dpp<0x4e, LV0 + 3>(x);     // quad_perm [2,3,0,1]
    reduce_stage_dpp<0x124, LV0 + 4>(x);    // row_ror:4
    reduce_stage_dpp<0x128, LV0 + 5>(x);    // row_ror:8
    const uint32_t sh = ((uint32_t)lane & 14u) << 1;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < (kOut + 7) / 8; ++g) {   // digits 8g .. 8g + 7: byte p of acc = those bits of position p's count
        uint32_t acc = 0u;
#pragma unroll
        for (int l = 8 * g; l < 8 * g + 8 && l < kOut; ++l) {
            const uint32_t n = (x[l] >> sh) & 15u;
            acc |= (n * (0x00204081u << (l & 7))) & (0x01010101u << (l & 7));
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] |= ((acc >> (8 * p)) & 0xffu) << (8 * g);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) cnt[p] = (int32_t)v[p];
}

// the STATS all-reduce (sum of squares, max |v|) over the wave with the same moves: every lane gets the totals
template <int CTRL>
__device__ __forceinline__ void sum_max_stage_dpp(unsigned long long& ss, uint32_t& mx) {
    ss += ((unsigned long long)dpp_mov<CTRL>((uint32_t)(ss >> 32)) << 32) | dpp_mov<CTRL>((uint32_t)ss);
    const uint32_t o = dpp_mov<CTRL>(mx);
    mx = o > mx ? o : mx;
}

template <bool SWAP32>
__device__ __forceinline__ void sum_max_stage_swap(unsigned long long& ss, uint32_t& mx) {
    const uint32_t l = (uint32_t)ss, h = (uint32_t)(ss >> 32);
    const auto rl = SWAP32 ? __builtin_amdgcn_permlane32_swap(l, l, false, false) : __builtin_amdgcn_permlane16_swap(l, l, false, false);
    const auto rh = SWAP32 ? __builtin_amdgcn_permlane32_swap(h, h, false, false) : __builtin_amdgcn_permlane16_swap(h, h, false, false);
    const auto rm = SWAP32 ? __builtin_amdgcn_permlane32_swap(mx, mx, false, false) : __builtin_amdgcn_permlane16_swap(mx, mx, false, false);
    ss = (((unsigned long long)rh[0] << 32) | rl[0]) + (((unsigned long long)rh[1] << 32) | rl[1]);
    mx = rm[0] > rm[1] ? rm[0] : rm[1];
}

__device__ __forceinline__ void wave_sum_max_valu(unsigned long long& ss, uint32_t& mx) {
    sum_max_stage_dpp<0xb1>(ss, mx);
    sum_max_stage_dpp<0x4e>(ss, mx);
    sum_max_stage_dpp<0x141>(ss, mx);
    sum_max_stage_dpp<0x140>(ss, mx);
    sum_max_stage_swap<false>(ss, mx);
    sum_max_stage_swap<true>(ss, mx);
}

// 256 threads = 4 waves, each wave owns BPW consecutive 64-dim blocks and streams over all hashes of
// one unit; a unit needs ny = ceil(nblk / (4*BPW)) workgroups.  1-D grid, XCD aware: workgroups are
// dealt round-robin over the 8 XCDs, so the ny workgroups of one unit are given linear ids 8 apart
// (same XCD, dispatched together) and share the unit's hashes through that XCD's L2:
//   id = (unit/8) * 8*ny + y*8 + unit%8.   Placement only affects HBM traffic, never results.
// STATS: also accumulate each sample's exact sum of squares (int64 atomics, one per wave) and the largest |v|
// of the launch -- for the units that are a whole sample (single) only, because a multi-unit sample's entries
// are only final once all its units have been added: the host runs k_stats over those rows afterwards.
//
// DEEP (variant 24): the carry-save tree reaches 128 hashes per lane before anything ripples.  The loop still hashes four
// batches per iteration and gets one weight-32 carry out of them; carries of weight 32 and 64 wait in p32 / p64 until a
// second one of the same weight exists, and the two are full-added into digit 5 / 6 at once.  A ripple (half adders through
// digits 7..10) follows once per 128 hashes instead of through 5..10 once per 32, so counting costs ~2.05 bitop3 per
// input word instead of ~2.45; the level-1 adder that also does the hash's last xor (absorb) adds 0.5 to either figure and
// takes the v_xor_b32 per input word of that xorshift away.  The branches on the iteration number are wave-uniform.  The
// epilogue is reduce_counts_wave4, which takes the four blocks of a wave: DEEP exists for BPW = 4 only.
//
// Main loop, VALU instructions per (hash, 64-dim block) as compiled (tools/check_project_isa.py): variant 24 19.38,
// 14 20.04, 12 21.27, 2 21.94, 1 22.12 (20.63 / 21.29 / 22.77 / 22.94 / 23.12 with the xorshift outside the adder and the
// shared round's 64-bit shift split in two).  The multiplies through mad64 leave these counts as they are and turn two
// v_add3_u32 per pair into v_add_u32 in variants 24, 2 and 1 (both rounds) and one in 14 and 12 (first round).  250 / 256
// VGPRs for BPW 4 (variant 24 / 14: two waves per SIMD), 138 / 137 for BPW 2 (three), 103 for BPW 1 (four); no AGPRs, no
// scratch.
template <int BPW, bool STATS, bool SHARED = false, bool DEEP = false>
__global__ __launch_bounds__(256) void k_project(const uint64_t* __restrict__ hashes,
                                                 const ProjUnit* __restrict__ units, long long n_units, int ny,
                                                 int d, int nblk, int32_t* __restrict__ out,
                                                 unsigned long long* __restrict__ sumsq,
                                                 unsigned long long* __restrict__ max_abs) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long grp = (long long)blockIdx.x / (8 * ny);
    const int rem = (int)((long long)blockIdx.x % (8 * ny));
    const long long unit = grp * 8 + (rem & 7);
    const int y = rem >> 3;
    if (unit >= n_units) return;
    const int b0 = (y * 4 + wave) * BPW;
    if (b0 >= nblk) return;
    const ProjUnit u = units[unit];
    const uint64_t* base = hashes + u.begin;
    const int64_t count = u.count;

    Acc<BPW> s;
#pragma unroll
    for (int b = 0; b < BPW; ++b)
#pragma unroll
        for (int l = 0; l < kLV; ++l) s.lo[b][l] = s.hi[b][l] = 0u;

    uint64_t cb[BPW];
#pragma unroll
    for (int b = 0; b < BPW; ++b) cb[b] = (uint64_t)(b0 + b) * 64ULL + kGolden;

    // Which instantiations take which multiply through mad64 (decided by an A/B on the flagship, LABNOTES round 10).  The second
    // multiply of the shared generator needs a register per block that holds zero: the DEEP kernel has room for them, the
    // other BPW-4 kernels (variant 14) would drop to one wave per SIMD and keep the first round alone.  The general generator
    // uses the same registers, so it follows wherever they exist or cost no wave (variants 24, 2 and 1).
    constexpr bool kRound2 = SHARED && DEEP;
    constexpr bool kMadGeneral = !SHARED || kRound2;
    // The zero low halves of the addends {0, cross} (mul64_mad, BatchGenShared): opaque to the compiler, which would write a
    // fresh zero in front of every multiply if it knew the value.  The statements are identical and have no inputs, so the
    // compiler is free to merge or rematerialise them; that it keeps one register per block, written once, and pays no move
    // for them is a property of the machine code, held by tests/test_project_mad_isa_cpu.py (v_mov_b32 per pair), not of
    // this source.  Any outcome computes the same values.  Where no multiply uses them they are plain zeros, never read.
    uint32_t zero[BPW];
#pragma unroll
    for (int b = 0; b < BPW; ++b) {
        if constexpr (kRound2 || kMadGeneral) asm("v_mov_b32 %0, 0" : "=v"(zero[b]));
        else zero[b] = 0u;
    }

    // Batches of 8 hashes per lane (512 per wave); batch i+1 is loaded while batch i is hashed.
    if (count > 0) {
        const int64_t last = count - 1;
        const int64_t nfull = count >> 9;
        uint64_t hv[8], hn[8];
        load_batch<true>(hv, base, 0, lane, last);
        int64_t b = 0;
        // four batches = 32 hashes per lane: Harley-Seal tree of depth 5, then one ripple (DEEP: see above).  The loop
        // takes every full group of four batches.  Its prefetches have no bounds handling: the last one of the unit's last
        // group reads the 512 hashes behind the unit -- the next unit's, which the masked tail ignores -- unless the host
        // saw that they end outside the hash array (kProjTailGuard): then that group is left to the clamped path below.
        uint32_t p32lo[BPW], p32hi[BPW], p64lo[BPW], p64hi[BPW];
        int grp4 = 0;   // DEEP: iterations done; bit 0 / 1 = a weight-32 / weight-64 carry is pending
        const int64_t nloop = (u.flags & kProjTailGuard) ? nfull - 1 : nfull;
        for (; b + 4 <= nloop; b += 4) {
            uint32_t c8lo[4][BPW], c8hi[4][BPW];
#pragma unroll
            for (int sb = 0; sb < 4; ++sb) {
                load_batch<false>(hn, base, (b + sb + 1) << 9, lane, last);
                uint64_t xv[8];
                if (SHARED && !hazard(hv, cb[0], xv)) {
                    BatchGenShared<BPW, kRound2> g(xv, zero);
                    absorb<3, BPW>(s, g, c8lo[sb], c8hi[sb]);
                } else {
                    BatchGen<BPW, false, kMadGeneral> g(hv, cb, zero, 0);
                    absorb<3, BPW>(s, g, c8lo[sb], c8hi[sb]);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) hv[j] = hn[j];
            }
            uint32_t c16lo[2][BPW], c16hi[2][BPW], c32lo[BPW], c32hi[BPW];
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                for (int q = 0; q < BPW; ++q) {
                    const uint32_t tl = s.lo[q][3], th = s.hi[q][3];
                    c16lo[h2][q] = maj3(tl, c8lo[2 * h2][q], c8lo[2 * h2 + 1][q]);
                    c16hi[h2][q] = maj3(th, c8hi[2 * h2][q], c8hi[2 * h2 + 1][q]);
                    s.lo[q][3] = xor3(tl, c8lo[2 * h2][q], c8lo[2 * h2 + 1][q]);
                    s.hi[q][3] = xor3(th, c8hi[2 * h2][q], c8hi[2 * h2 + 1][q]);
                }
#pragma unroll
            for (int q = 0; q < BPW; ++q) {
                const uint32_t tl = s.lo[q][4], th = s.hi[q][4];
                c32lo[q] = maj3(tl, c16lo[0][q], c16lo[1][q]);
                c32hi[q] = maj3(th, c16hi[0][q], c16hi[1][q]);
                s.lo[q][4] = xor3(tl, c16lo[0][q], c16lo[1][q]);
                s.hi[q][4] = xor3(th, c16hi[0][q], c16hi[1][q]);
            }
            if constexpr (DEEP) {
                if (grp4 & 1) {
                    uint32_t c64lo[BPW], c64hi[BPW];
#pragma unroll
                    for (int q = 0; q < BPW; ++q) {
                        const uint32_t tl = s.lo[q][5], th = s.hi[q][5];
                        c64lo[q] = maj3(tl, p32lo[q], c32lo[q]);
                        c64hi[q] = maj3(th, p32hi[q], c32hi[q]);
                        s.lo[q][5] = xor3(tl, p32lo[q], c32lo[q]);
                        s.hi[q][5] = xor3(th, p32hi[q], c32hi[q]);
                    }
                    if (grp4 & 2) {
                        uint32_t c128lo[BPW], c128hi[BPW];
#pragma unroll
                        for (int q = 0; q < BPW; ++q) {
                            const uint32_t tl = s.lo[q][6], th = s.hi[q][6];
                            c128lo[q] = maj3(tl, p64lo[q], c64lo[q]);
                            c128hi[q] = maj3(th, p64hi[q], c64hi[q]);
                            s.lo[q][6] = xor3(tl, p64lo[q], c64lo[q]);
                            s.hi[q][6] = xor3(th, p64hi[q], c64hi[q]);
                        }
                        ripple<7, BPW>(s, c128lo, c128hi);
                    } else {
#pragma unroll
                        for (int q = 0; q < BPW; ++q) p64lo[q] = c64lo[q], p64hi[q] = c64hi[q];
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < BPW; ++q) p32lo[q] = c32lo[q], p32hi[q] = c32hi[q];
                }
                ++grp4;
            } else {
                ripple<5, BPW>(s, c32lo, c32hi);
            }
        }
        if constexpr (DEEP) {   // the pending carries go in before anything of weight 1 is added again
            if (grp4 & 1) ripple<5, BPW>(s, p32lo, p32hi);
            if (grp4 & 2) ripple<6, BPW>(s, p64lo, p64hi);
        }
        // leftover full batches
        for (; b < nfull; ++b) {
            load_batch<true>(hn, base, (b + 1) << 9, lane, last);
            BatchGen<BPW, false, kMadGeneral> g(hv, cb, zero, 0);
            uint32_t clo[BPW], chi[BPW];
            absorb<3, BPW>(s, g, clo, chi);
            ripple<3, BPW>(s, clo, chi);
#pragma unroll
            for (int j = 0; j < 8; ++j) hv[j] = hn[j];
        }
        // partial last batch, masked; only as many of its 8 hash slots are evaluated as hold anything (a sample of
        // 100 hashes needs 2 of them, not 8)
        if ((count & 511) != 0) {
            const int rem = (int)(count & 511);
            BatchGen<BPW, true, kMadGeneral> g(hv, cb, zero, count - (nfull << 9) - lane);
            uint32_t clo[BPW], chi[BPW];
            if (rem <= 64) {
                absorb<0, BPW>(s, g, clo, chi);
                ripple<0, BPW>(s, clo, chi);
            } else if (rem <= 128) {
                absorb<1, BPW>(s, g, clo, chi);
                ripple<1, BPW>(s, clo, chi);
            } else if (rem <= 256) {
                absorb<2, BPW>(s, g, clo, chi);
                ripple<2, BPW>(s, clo, chi);
            } else {
                absorb<3, BPW>(s, g, clo, chi);
                ripple<3, BPW>(s, clo, chi);
            }
        }
    }

    long long ss = 0;
    unsigned int mx = 0;
    static_assert(!DEEP || BPW == 4, "the DEEP epilogue reduces four blocks together");
    if constexpr (DEEP) {
        // one reduction over the wave's four blocks (reduce_counts_wave4): this lane holds four consecutive entries of one
        // block.  Blocks behind nblk were hashed like the others and are dropped here: k < d implies block < nblk.
        int32_t cnt[4];
        if (count <= 64) reduce_counts_wave4<1>(s, lane, cnt);
        else if (count <= 64 * 15) reduce_counts_wave4<4>(s, lane, cnt);
        else if (count <= 64 * 127) reduce_counts_wave4<7>(s, lane, cnt);
        else if (count <= 64 * 511) reduce_counts_wave4<9>(s, lane, cnt);
        else if (count <= 64 * 1023) reduce_counts_wave4<10>(s, lane, cnt);
        else reduce_counts_wave4<kLV>(s, lane, cnt);
        const int row = lane >> 4;
        const int k0 = (b0 + (row & 1) + 2 * (lane & 1)) * 64 + 32 * (row >> 1) + 4 * ((lane & 15) >> 1);
        int32_t v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) v[p] = (int32_t)count - 2 * cnt[p];
        int32_t* dst = out + (int64_t)u.sample * d + k0;
        // d a multiple of 4 and a 16-byte aligned base: every row is aligned and k0 .. k0 + 3 are inside the row together,
        // so the eight lanes of a block's half write 128 contiguous bytes with one store each
        if (u.single && (d & 3) == 0 && ((uintptr_t)out & 15) == 0) {
            if (k0 < d) *reinterpret_cast<int4*>(dst) = make_int4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (k0 + p < d) {
                    if (u.single)
                        dst[p] = v[p];
                    else
                        atomicAdd(dst + p, v[p]);
                }
            }
        }
        if (STATS) {   // (of a unit that is not single: never used)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (k0 + p < d) {
                    ss += (long long)v[p] * v[p];
                    const unsigned int av = (unsigned int)(v[p] < 0 ? -v[p] : v[p]);
                    mx = av > mx ? av : mx;
                }
            }
        }
    } else {
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            if (b0 + b >= nblk) break;
            int32_t cnt;   // a lane absorbed at most ceil(count / 64) hashes
            if (count <= 64) cnt = reduce_counts<1>(s.lo[b], s.hi[b], lane);
            else if (count <= 64 * 15) cnt = reduce_counts<4>(s.lo[b], s.hi[b], lane);
            else if (count <= 64 * 127) cnt = reduce_counts<7>(s.lo[b], s.hi[b], lane);
            else if (count <= 64 * 511) cnt = reduce_counts<9>(s.lo[b], s.hi[b], lane);
            else cnt = reduce_counts<kLV>(s.lo[b], s.hi[b], lane);
            const int k = (b0 + b) * 64 + lane;
            if (k < d) {
                const int32_t v = (int32_t)count - 2 * cnt;
                int32_t* dst = out + (int64_t)u.sample * d + k;
                if (u.single)
                    *dst = v;
                else
                    atomicAdd(dst, v);
                if (STATS) {   // (of a unit that is not single: never used)
                    ss += (long long)v * v;
                    const unsigned int av = (unsigned int)(v < 0 ? -v : v);
                    mx = av > mx ? av : mx;
                }
            }
        }
    }
    if (STATS && u.single) {
        if constexpr (DEEP) {
            unsigned long long uss = (unsigned long long)ss;   // two's complement: the wrapped sum is the same
            uint32_t umx = mx;
            wave_sum_max_valu(uss, umx);
            ss = (long long)uss;
            mx = umx;
        } else {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                ss += __shfl_xor(ss, o, 64);
                const unsigned int other = (unsigned int)__shfl_xor((int)mx, o, 64);
                mx = other > mx ? other : mx;
            }
        }
        if (lane == 0) {
            atomicAdd(sumsq + u.sample, (unsigned long long)ss);
            // the running maximum only grows: look before bumping it (one atomic per wave on ONE address
            // serialises at the L2 -- 1.6e7 of them cost 160 ms on a million small samples)
            if (mx > *reinterpret_cast<volatile unsigned long long*>(max_abs)) atomicMax(max_abs, (unsigned long long)mx);
        }
    }
}

// one wave per sketch row: exact int64 sum of squares
__global__ __launch_bounds__(256) void k_sumsq(const int32_t* __restrict__ sk, int64_t n, int d,
                                               int64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int32_t* p = sk + row * d;
    long long acc = 0;
    for (int k = lane; k < d; k += 64) {
        const long long v = p[k];
        acc += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) out[row] = acc;
}

// one wave per sketch row: exact int64 sum of squares AND the largest |v| of the whole array (one pass)
__global__ __launch_bounds__(256) void k_stats(const int32_t* __restrict__ sk, int64_t n, int d,
                                               int64_t* __restrict__ sumsq, unsigned long long* __restrict__ max_abs) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int32_t* p = sk + row * d;
    long long acc = 0;
    unsigned int m = 0;
    if ((d & 3) == 0 && ((uintptr_t)p & 15) == 0) {
        const int4* p4 = reinterpret_cast<const int4*>(p);
        for (int k = lane; k < d / 4; k += 64) {
            const int4 v = p4[k];
            const long long a = v.x, b = v.y, c = v.z, e = v.w;
            acc += a * a + b * b + c * c + e * e;
            const unsigned int ma = (unsigned int)(a < 0 ? -a : a), mb = (unsigned int)(b < 0 ? -b : b);
            const unsigned int mc = (unsigned int)(c < 0 ? -c : c), me = (unsigned int)(e < 0 ? -e : e);
            m = max(max(m, max(ma, mb)), max(mc, me));
        }
    } else {
        for (int k = lane; k < d; k += 64) {
            const long long v = p[k];
            acc += v * v;
            m = max(m, (unsigned int)(v < 0 ? -v : v));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        m = max(m, (unsigned int)__shfl_xor((int)m, o, 64));
    }
    if (lane == 0) {
        sumsq[row] = acc;
        if (m > *reinterpret_cast<volatile unsigned long long*>(max_abs)) atomicMax(max_abs, (unsigned long long)m);
    }
}

__global__ __launch_bounds__(256) void k_saturate_i16(const int32_t* __restrict__ in, int64_t n,
                                                      int16_t* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int32_t v = in[i];
        out[i] = (int16_t)(v > 32767 ? 32767 : (v < -32768 ? -32768 : v));
    }
}

}  // namespace

// variant: 1 / 2 = that many 64-dim blocks per wave, every block hashed on its own; 12 / 14 = two / four blocks per wave
// with the shared first splitmix64 round (BatchGenShared); 24 = 14 with the deeper carry-save tree and the VALU epilogue
// (DEEP)
template <int BPW, bool SHARED, bool DEEP = false>
static void launch_project_as(hipStream_t stream, unsigned grid, bool stats, const uint64_t* d_hashes, const ProjUnit* d_units,
                              long long nu, int ny, int d, int nblk, int32_t* d_out, unsigned long long* d_sumsq,
                              unsigned long long* d_max_abs) {
    if (stats)
        hipLaunchKernelGGL((k_project<BPW, true, SHARED, DEEP>), dim3(grid), dim3(256), 0, stream, d_hashes, d_units, nu, ny, d, nblk,
                           d_out, d_sumsq, d_max_abs);
    else
        hipLaunchKernelGGL((k_project<BPW, false, SHARED, DEEP>), dim3(grid), dim3(256), 0, stream, d_hashes, d_units, nu, ny, d, nblk,
                           d_out, d_sumsq, d_max_abs);
}

template <int BPW, bool SHARED, bool DEEP = false>
static int project_blocks_as(bool stats) {
    int nb = 0;
    const hipError_t e = stats ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_project<BPW, true, SHARED, DEEP>, 256, 0)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_project<BPW, false, SHARED, DEEP>, 256, 0);
    return e == hipSuccess ? nb : -1;
}

int project_blocks_per_cu(int variant, bool stats) {
    switch (variant) {
        case 1: return project_blocks_as<1, false>(stats);
        case 12: return project_blocks_as<2, true>(stats);
        case 24: return project_blocks_as<4, true, true>(stats);
        case 14: return project_blocks_as<4, true>(stats);
        default: return project_blocks_as<2, false>(stats);
    }
}

int launch_project(hipStream_t stream, const uint64_t* d_hashes, const ProjUnit* d_units, int64_t n_units,
                   int d, int32_t* d_out, int variant, unsigned long long* d_sumsq, unsigned long long* d_max_abs) {
    if (n_units == 0) return 0;
    const int nblk = (d + 63) / 64;
    const int bpw = variant % 10;
    const int ny = (nblk + 4 * bpw - 1) / (4 * bpw);
    // a dispatch holds at most 2^32 work-items per dimension: slabs of at most ~2^32/256 workgroups
    const int64_t kMaxUnits = ((int64_t)(0xffffffffLL / 256) / (8 * ny) - 1) * 8;
    for (int64_t u0 = 0; u0 < n_units; u0 += kMaxUnits) {
        const int64_t nu = n_units - u0 < kMaxUnits ? n_units - u0 : kMaxUnits;
        const unsigned grid = (unsigned)(((nu + 7) / 8) * 8 * ny);
        const bool stats = d_sumsq != nullptr;
        switch (variant) {
            case 1: launch_project_as<1, false>(stream, grid, stats, d_hashes, d_units + u0, (long long)nu, ny, d, nblk, d_out, d_sumsq, d_max_abs); break;
            case 12: launch_project_as<2, true>(stream, grid, stats, d_hashes, d_units + u0, (long long)nu, ny, d, nblk, d_out, d_sumsq, d_max_abs); break;
            case 24: launch_project_as<4, true, true>(stream, grid, stats, d_hashes, d_units + u0, (long long)nu, ny, d, nblk, d_out, d_sumsq, d_max_abs); break;
            case 14: launch_project_as<4, true>(stream, grid, stats, d_hashes, d_units + u0, (long long)nu, ny, d, nblk, d_out, d_sumsq, d_max_abs); break;
            default: launch_project_as<2, false>(stream, grid, stats, d_hashes, d_units + u0, (long long)nu, ny, d, nblk, d_out, d_sumsq, d_max_abs); break;
        }
    }
    return 0;
}

// one wave per row, 4 rows per workgroup; slabs of 2^22 workgroups keep each dispatch below 2^32 work-items
constexpr int64_t kRowSlab = (int64_t)4 << 22;

int launch_sumsq(hipStream_t stream, const int32_t* d_sk, int64_t n, int d, int64_t* d_out) {
    for (int64_t r0 = 0; r0 < n; r0 += kRowSlab) {
        const int64_t m = n - r0 < kRowSlab ? n - r0 : kRowSlab;
        hipLaunchKernelGGL(k_sumsq, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, d_sk + r0 * d, m, d, d_out + r0);
    }
    return 0;
}

int launch_stats(hipStream_t stream, const int32_t* d_sk, int64_t n, int d, int64_t* d_sumsq,
                 unsigned long long* d_max_abs) {
    for (int64_t r0 = 0; r0 < n; r0 += kRowSlab) {
        const int64_t m = n - r0 < kRowSlab ? n - r0 : kRowSlab;
        hipLaunchKernelGGL(k_stats, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, d_sk + r0 * d, m, d, d_sumsq + r0,
                           d_max_abs);
    }
    return 0;
}

int launch_saturate_i16(hipStream_t stream, const int32_t* d_in, int64_t n, int16_t* d_out) {
    if (n == 0) return 0;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_saturate_i16, dim3((unsigned)blocks), dim3(256), 0, stream, d_in, n, d_out);
    return 0;
}

}  // namespace mvs
