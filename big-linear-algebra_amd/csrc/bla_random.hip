// bla_random.hip -- counter-based device random numbers (Philox4x32-10, bla_philox.h): uniform 32-bit words, normals, Bernoulli decisions, and a
// permutation (the stable argsort of a stream of words).
//
// Not in the reference (its U-Net draws dropout decisions and noise from libc rand(), one call per element on the host).  Every value is a pure
// function of (seed, offset, element index), so a stream can be restated anywhere -- tests/test_diffusion_gpu.py does it in numpy -- and any
// slice of it can be drawn on its own.  The kernels are HBM-store-bound: each lane produces whole Philox blocks and writes 16 bytes at a time
// (4 words / normals, 16 decisions); a scalar head and tail take the elements in front of the first 16-byte boundary and behind the last.
#include "bla_internal.h"
#include "bla_philox.h"
#include <cmath>

namespace bla {
namespace {

constexpr int kThreads = 256;
enum { KIND_U32 = 0, KIND_NORMAL = 1, KIND_BERNOULLI = 2 };

struct RandArgs {
	unsigned long long seed, offset;
	float mean, stddev;          // normal
	unsigned long long thr;      // Bernoulli: 1 = w < thr, thr = floor(p * 2^32) in [0, 2^32]
};

template <int KIND> struct Kind;
template <> struct Kind<KIND_U32> { using T = uint32_t; static constexpr uint32_t tag = PHILOX_TAG_U32; };
template <> struct Kind<KIND_NORMAL> { using T = float; static constexpr uint32_t tag = PHILOX_TAG_NORMAL; };
template <> struct Kind<KIND_BERNOULLI> { using T = uint8_t; static constexpr uint32_t tag = PHILOX_TAG_BERNOULLI; };

// the four values of Philox block j of the stream
template <int KIND>
__device__ __forceinline__ void block_values(const RandArgs& a, unsigned long long j, typename Kind<KIND>::T* v) {
	const uint4 w = philox_block(a.seed, j, Kind<KIND>::tag);
	if constexpr (KIND == KIND_U32) {
		v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
	} else if constexpr (KIND == KIND_NORMAL) {
		const float4 z = philox_normal4(w);
		v[0] = a.mean + a.stddev * z.x; v[1] = a.mean + a.stddev * z.y; v[2] = a.mean + a.stddev * z.z; v[3] = a.mean + a.stddev * z.w;
	} else {
		v[0] = (unsigned long long)w.x < a.thr; v[1] = (unsigned long long)w.y < a.thr; v[2] = (unsigned long long)w.z < a.thr; v[3] = (unsigned long long)w.w < a.thr;
	}
}

// Elements [head, head + chunks * E) in 16-byte chunks (E = 16 / sizeof(T) values, the first at a 16-byte aligned address); SH = head % 4 is where a
// chunk starts inside its first Philox block, so a chunk takes (SH + E + 3) / 4 blocks.  Elements [0, head) and [head + chunks * E, n) go one per lane.
template <int KIND, int SH>
__global__ void __launch_bounds__(kThreads) rand_kernel(typename Kind<KIND>::T* __restrict__ out, size_t n, size_t head, size_t chunks, RandArgs a) {
	using T = typename Kind<KIND>::T;
	constexpr int E = 16 / sizeof(T), NB = (SH + E + 3) / 4;
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	for (size_t q = tid; q < chunks; q += stride) {
		const size_t e0 = head + q * E;
		T v[4 * NB];
#pragma unroll
		for (int b = 0; b < NB; b++) block_values<KIND>(a, a.offset + e0 / 4 + b, v + 4 * b);
		union { T t[E]; uint4 u; } pack;
#pragma unroll
		for (int k = 0; k < E; k++) pack.t[k] = v[SH + k];
		*reinterpret_cast<uint4*>(out + e0) = pack.u;
	}
	const size_t body_end = head + chunks * E, tail = n - body_end;
	if (tid < head + tail) {
		const size_t e = tid < head ? tid : body_end + (tid - head);
		T v[4];
		block_values<KIND>(a, a.offset + e / 4, v);
		const int w = (int)(e % 4);
		out[e] = w == 0 ? v[0] : w == 1 ? v[1] : w == 2 ? v[2] : v[3];
	}
}

template <int KIND>
bla_status launch_rand(void* stream, typename Kind<KIND>::T* out, size_t n, const RandArgs& a) {
	using T = typename Kind<KIND>::T;
	bla_status st = require_ready();
	if (st) return st;
	if (n == 0) return BLA_OK;
	BLA_REQUIRE(out, BLA_ERR_INVALID, "null output");
	BLA_REQUIRE((uintptr_t)out % sizeof(T) == 0, BLA_ERR_INVALID, "output not aligned to its element size");
	constexpr size_t E = 16 / sizeof(T);
	size_t head = ((16 - (uintptr_t)out % 16) % 16) / sizeof(T);
	if (head > n) head = n;
	const size_t chunks = (n - head) / E;
	const size_t cap = 8 * (size_t)(ctx().num_cus > 0 ? ctx().num_cus : 256);
	size_t blocks = (chunks + kThreads - 1) / kThreads;
	blocks = blocks < 1 ? 1 : (blocks > cap ? cap : blocks);
	hipStream_t s = pick_stream(stream);
	switch (head % 4) {   // head + tail < 2 E <= 32 elements: the first workgroup always covers them
		case 0: hipLaunchKernelGGL((rand_kernel<KIND, 0>), dim3((unsigned)blocks), dim3(kThreads), 0, s, out, n, head, chunks, a); break;
		case 1: hipLaunchKernelGGL((rand_kernel<KIND, 1>), dim3((unsigned)blocks), dim3(kThreads), 0, s, out, n, head, chunks, a); break;
		case 2: hipLaunchKernelGGL((rand_kernel<KIND, 2>), dim3((unsigned)blocks), dim3(kThreads), 0, s, out, n, head, chunks, a); break;
		default: hipLaunchKernelGGL((rand_kernel<KIND, 3>), dim3((unsigned)blocks), dim3(kThreads), 0, s, out, n, head, chunks, a); break;
	}
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

// The stable ascending argsort of keys [n] by counting: lane i holds key i, every workgroup streams all keys through LDS in tiles (each LDS read is
// one address for the whole wave: a broadcast), rank_i = #{j : key_j < key_i or (key_j == key_i and j < i)} -- one 64-bit compare of (key, index)
// pairs -- and out[rank_i] = i.  The pairs are distinct, so the ranks are a permutation of 0 .. n-1: every store lands inside out [n], and no two
// lanes write the same element.  O(n^2) compares, meant for a shuffle once per epoch.
constexpr int kRankTile = 2048;
__global__ void __launch_bounds__(kThreads) rank_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ out) {
	__shared__ uint32_t tile[kRankTile];
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const unsigned long long mine = i < n ? ((unsigned long long)keys[i] << 32) | i : 0;
	uint32_t rank = 0;
	for (uint32_t base = 0; base < n; base += kRankTile) {
		const uint32_t count = n - base < (uint32_t)kRankTile ? n - base : (uint32_t)kRankTile;
		__syncthreads();
		for (uint32_t k = threadIdx.x; k < count; k += blockDim.x) tile[k] = keys[base + k];
		__syncthreads();
		for (uint32_t k = 0; k < count; k++) rank += ((((unsigned long long)tile[k] << 32) | (base + k)) < mine);
	}
	if (i < n) out[rank] = i;
}

}  // namespace
}  // namespace bla

using namespace bla;

extern "C" {

bla_status bla_rand_u32(void* stream, unsigned int* d_out, size_t n, unsigned long long seed, unsigned long long offset) {
	RandArgs a = {seed, offset, 0.f, 0.f, 0};
	return launch_rand<KIND_U32>(stream, d_out, n, a);
}

bla_status bla_rand_normal_f32(void* stream, float* d_out, size_t n, float mean, float stddev, unsigned long long seed, unsigned long long offset) {
	RandArgs a = {seed, offset, mean, stddev, 0};
	return launch_rand<KIND_NORMAL>(stream, d_out, n, a);
}

bla_status bla_rand_bernoulli_u8(void* stream, unsigned char* d_out, size_t n, float p, unsigned long long seed, unsigned long long offset) {
	BLA_REQUIRE(!std::isnan(p), BLA_ERR_INVALID, "p is NaN");
	const double t = std::floor((double)p * 4294967296.0);
	RandArgs a = {seed, offset, 0.f, 0.f, (unsigned long long)(t < 0 ? 0.0 : (t > 4294967296.0 ? 4294967296.0 : t))};
	return launch_rand<KIND_BERNOULLI>(stream, d_out, n, a);
}

bla_status bla_rand_permutation_u32(void* stream, unsigned int* d_out, unsigned int* d_keys, size_t n, unsigned long long seed, unsigned long long offset) {
	bla_status st = require_ready();
	if (st) return st;
	if (n == 0) return BLA_OK;
	BLA_REQUIRE(n <= ((size_t)1 << 20), BLA_ERR_INVALID, "n %zu > 2^20", n);
	BLA_REQUIRE(d_out && d_keys && d_out != d_keys && (uintptr_t)d_out % 4 == 0, BLA_ERR_INVALID, "outputs null, the same or not 4-byte aligned");
	if ((st = bla_rand_u32(stream, d_keys, n, seed, offset))) return st;
	hipLaunchKernelGGL(rank_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, pick_stream(stream), (const uint32_t*)d_keys, (uint32_t)n, d_out);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

}  // extern "C"
