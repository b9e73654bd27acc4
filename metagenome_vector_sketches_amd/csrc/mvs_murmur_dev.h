// mvs_murmur_dev.h -- device pieces of MurmurHash3_x64_128 that the hashing kernels share (mvs_kmer.hip: DNA k-mers,
// mvs_protein.hip: residues): the 64-bit multiplies by constants as one v_mad_u64_u32 with the cross terms in the addend (the
// idiom of mvs_project.hip), the finaliser, the two key mixes and one whole 16-byte block.  Every function is inlined into
// the kernel that calls it; the anonymous namespace keeps each unit's copy its own.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace mvs {

namespace {

constexpr uint64_t kMurC1 = 0x87c37b91114253d5ULL, kMurC2 = 0x4cf5ad432745937fULL;
constexpr uint64_t kFmix1 = 0xff51afd7ed558ccdULL, kFmix2 = 0xc4ceb9fe1a85ec53ULL;

// a * b + c as one v_mad_u64_u32 (b a constant in an SGPR; the carry out goes to an SGPR pair nobody reads)
__device__ __forceinline__ uint64_t mad64(uint32_t a, uint32_t b, uint64_t c) {
    uint64_t r, carry;
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(carry) : "v"(a), "s"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t mul_lo(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_mul_lo_u32 %0, %1, %2" : "=v"(r) : "v"(a), "s"(b));
    return r;
}
// z * C (mod 2^64) for a constant C: lo * C.lo + ((lo * C.hi + hi * C.lo) << 32), the cross terms in the mad's addend
__device__ __forceinline__ uint64_t mul64_mad(uint64_t z, uint64_t C) {
    const uint32_t zl = (uint32_t)z, zh = (uint32_t)(z >> 32);
    const uint32_t cross = mul_lo(zl, (uint32_t)(C >> 32)) + mul_lo(zh, (uint32_t)C);
    return mad64(zl, (uint32_t)C, (uint64_t)cross << 32);
}
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k = mul64_mad(k, kFmix1);
    k ^= k >> 33;
    k = mul64_mad(k, kFmix2);
    return k ^ (k >> 33);
}
__device__ __forceinline__ uint64_t mur_k1(uint64_t k1) { return mul64_mad(rotl64(mul64_mad(k1, kMurC1), 31), kMurC2); }
__device__ __forceinline__ uint64_t mur_k2(uint64_t k2) { return mul64_mad(rotl64(mul64_mad(k2, kMurC2), 33), kMurC1); }

// one whole 16-byte block: the words k1, k2 into the state
__device__ __forceinline__ void murmur_block(uint64_t& h1, uint64_t& h2, uint64_t k1, uint64_t k2) {
    h1 ^= mur_k1(k1);
    h1 = rotl64(h1, 27) + h2;
    h1 = h1 * 5 + 0x52dce729u;
    h2 ^= mur_k2(k2);
    h2 = rotl64(h2, 31) + h1;
    h2 = h2 * 5 + 0x38495ab5u;
}

}  // namespace

}  // namespace mvs
