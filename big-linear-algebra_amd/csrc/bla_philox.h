// bla_philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the stream layout of
// include/bla.h's counter-based generators, shared by bla_random.hip and bla_diffusion.hip.
//
// Stream (seed, offset, tag): element i is word i % 4 of the Philox block j = offset + i / 4 (64-bit), counter {lo(j), hi(j), tag, 0},
// key {lo(seed), hi(seed)}.  tag 0 = u32, 1 = normal, 2 = Bernoulli: the three streams of one (seed, offset) never share a block.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace bla {

enum { PHILOX_TAG_U32 = 0, PHILOX_TAG_NORMAL = 1, PHILOX_TAG_BERNOULLI = 2 };

__host__ __device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
	for (int r = 0; r < 10; r++) {
		if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
		const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
		c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0);
	}
	return c;
}

// the four words of block j of stream (seed, tag)
__device__ __forceinline__ uint4 philox_block(unsigned long long seed, unsigned long long j, uint32_t tag) {
	return philox4x32_10(make_uint4((uint32_t)j, (uint32_t)(j >> 32), tag, 0u), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Box-Muller on the word pairs (w0, w1) and (w2, w3): u = ((w >> 8) + 0.5) * 2^-24 in fp32 (in (0, 1]; the top values round to 1),
// r = sqrt(-2 ln u_a), z_a = r cos(2 pi u_b), z_b = r sin(2 pi u_b).  Accurate logf / sincospif: a numpy restatement stays within a few ulp.
__device__ __forceinline__ float philox_unit(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 0x1p-24f; }
__device__ __forceinline__ float4 philox_normal4(uint4 w) {
	float s0, c0, s1, c1;
	const float r0 = sqrtf(-2.0f * logf(philox_unit(w.x))), r1 = sqrtf(-2.0f * logf(philox_unit(w.z)));
	sincospif(2.0f * philox_unit(w.y), &s0, &c0);
	sincospif(2.0f * philox_unit(w.w), &s1, &c1);
	return make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
}
__device__ __forceinline__ float normal_at(unsigned long long seed, unsigned long long offset, size_t i) {
	const float4 z = philox_normal4(philox_block(seed, offset + i / 4, PHILOX_TAG_NORMAL));
	const int w = (int)(i % 4);
	return w == 0 ? z.x : w == 1 ? z.y : w == 2 ? z.z : z.w;
}
__device__ __forceinline__ uint32_t u32_at(unsigned long long seed, unsigned long long offset, size_t i, uint32_t tag = PHILOX_TAG_U32) {
	const uint4 u = philox_block(seed, offset + i / 4, tag);
	const int w = (int)(i % 4);
	return w == 0 ? u.x : w == 1 ? u.y : w == 2 ? u.z : u.w;
}

}  // namespace bla
