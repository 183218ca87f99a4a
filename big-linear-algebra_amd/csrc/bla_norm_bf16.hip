// bla_norm_bf16.hip -- group norm and its gradient with a channel-last bf16 output (include/bla.h, "group norm into a bf16 map").
//
// The bf16 convolutions gather from a padded channel-last map [B][Hp][Wp][Cp]; inside a ResNet block that map is the output of a group norm, which the fp32
// family writes planar.  The two entries here run the fp32 family's arithmetic (csrc/bla_group_norm.hip, quirk Q3 kept: `stdevs` holds the variance and the
// output is divided by it) and store the result where the next product reads it -- the store contract of bla_conv2d_gathered_bf16_chained.
//   * stats launch: one 1024-thread workgroup per (image, group).  fp64 sums in a fixed order (a thread's elements ascending, the wave by shuffles, the
//     sixteen waves ascending): the same call gives the same bits.  Forward: sum x and sum x^2 (x^2 is exact in fp64), m = (float)(sum x / n),
//     v = (float)((sum x^2 - 2 m sum x + n m^2) / n), the variance about the float m.  Gradient: A = (float)(sum s / n), B = (float)(sum nv s / n).
//   * apply launch (one kernel template for both entries): a workgroup takes 64 pixels of one image row x 64 channels.  It reads [c][x] (16-byte loads
//     when w % 4 == 0, every fp32 pointer is 16-byte aligned and d_drop 4-byte aligned, scalar loads otherwise), normalises every element with ITS channel's group statistics
//     (so an 8-channel chunk that straddles two groups is no special case), writes the optional planar fp32 output from the same registers, stages the
//     values in an fp32 LDS tile of pitch 65 and writes [x][c] as 16-byte chunks of 8 channels; channels from C up to Cp come out of the tile as +0.
//     Pitch 65 = 1 mod 32 (ds_read_b32 / ds_write_b32 bank on 32 dwords per 32-lane half): a half wave of the read phase holds 2 channels x 16 groups
//     of 4 pixels (bank c + x + j: 2-way, free on a 4-byte LDS store), of the write phase 8 chunks x 4 pixels (bank 8 cq + e + px: 2-way); pitch 64
//     would make the write phase's walk over a chunk's channels 8-way.  Only pixel positions are stored: halo, holes and guards keep
//     their bits.
#include "bla_internal.h"
#include "bla_bf16_tile.h"

namespace bla {
namespace {

constexpr int kStatThreads = 1024;

// every thread returns the same totals: lanes by shuffle, then the sixteen waves in ascending order
__device__ __forceinline__ void stat_block_sum(double& a, double& b) {
	__shared__ double sh[2][kStatThreads / 64];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
	if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
	__syncthreads();
	a = 0; b = 0;
	for (int i = 0; i < kStatThreads / 64; i++) { a += sh[0][i]; b += sh[1][i]; }
}

struct StatArgs { const float* x; const float* data; const float* means_in; const float* stdevs_in; float* out0; float* out1; int channels, group_size, groups, hw, vec; };

// DDX = false: x -> (means, stdevs) = (out0, out1) [batch][groups];  DDX = true: (source = x, data, means, stdevs) -> (A, B) = (out0, out1)
template <bool DDX>
__global__ __launch_bounds__(kStatThreads) void norm_bf16_stats_kernel(StatArgs p) {
	const int b = blockIdx.x / p.groups, g = blockIdx.x - b * p.groups, t = threadIdx.x;
	const int nch = min(p.group_size, p.channels - g * p.group_size);
	const size_t off = ((size_t)b * p.channels + (size_t)g * p.group_size) * p.hw;
	const long n = (long)nch * p.hw;
	const float m = DDX ? p.means_in[blockIdx.x] : 0.f, v = DDX ? p.stdevs_in[blockIdx.x] : 1.f;
	double a = 0, q = 0;
	if (p.vec) {   // hw % 4 == 0: a group starts on 16 bytes and holds whole float4s
#pragma unroll 4
		for (long i = 4L * t; i < n; i += 4L * kStatThreads) {
			const float4 s4 = *reinterpret_cast<const float4*>(p.x + off + i);
			const float s[4] = {s4.x, s4.y, s4.z, s4.w};
			if (DDX) {
				const float4 d4 = *reinterpret_cast<const float4*>(p.data + off + i);
				const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
				for (int e = 0; e < 4; e++) { const float nv = (d[e] - m) / v; a += s[e]; q += (double)nv * s[e]; }
			} else {
#pragma unroll
				for (int e = 0; e < 4; e++) { const double x = s[e]; a += x; q += x * x; }
			}
		}
	} else {
#pragma unroll 4
		for (long i = t; i < n; i += kStatThreads) {
			const float s = p.x[off + i];
			if (DDX) { const float nv = (p.data[off + i] - m) / v; a += s; q += (double)nv * s; }
			else { const double x = s; a += x; q += x * x; }
		}
	}
	stat_block_sum(a, q);
	if (t != 0) return;
	if (DDX) { p.out0[blockIdx.x] = (float)(a / (double)n); p.out1[blockIdx.x] = (float)(q / (double)n); return; }
	const float mean = (float)(a / (double)n);
	const double md = (double)mean;
	p.out0[blockIdx.x] = mean;
	p.out1[blockIdx.x] = (float)((q - 2.0 * md * a + (double)n * md * md) / (double)n);
}

struct ApplyArgs {
	const float* x;            // forward: the input; gradient: source
	const float* data;         // gradient only
	const unsigned char* drop; // forward only, optional
	const float* means; const float* stdevs; const float* ga; const float* gb;   // [batch][groups]; ga / gb: the gradient's A and B
	float* out;                // optional planar fp32 output
	bla_conv_bf16_map dst;     // dst.d optional
	int channels, group_size, groups, h, w, xtiles, vec;
};

template <bool DDX>
__global__ __launch_bounds__(256) void norm_bf16_apply_kernel(ApplyArgs a) {
	__shared__ float tile[64][65];
	const int xt = blockIdx.x % a.xtiles, ct = blockIdx.x / a.xtiles, y = blockIdx.y, b = blockIdx.z;
	const int c0 = ct * 64, x0 = xt * 64, xn = min(64, a.w - x0);
	const size_t plane = (size_t)a.h * a.w;
	for (int id = threadIdx.x; id < 64 * 16; id += 256) {
		const int c = id >> 4, x = (id & 15) * 4, cc = c0 + c;
		if (x >= xn) continue;
		const int cnt = min(4, xn - x);
		float r[4] = {0.f, 0.f, 0.f, 0.f};   // a channel from C up: +0
		if (cc < a.channels) {
			const size_t e = ((size_t)b * a.channels + cc) * plane + (size_t)y * a.w + x0 + x;
			const int gi = b * a.groups + cc / a.group_size;
			const float m = a.means[gi], v = a.stdevs[gi];
			const bool whole = a.vec && cnt == 4;
			float s[4] = {0.f, 0.f, 0.f, 0.f};
			if (whole) { const float4 q = *reinterpret_cast<const float4*>(a.x + e); s[0] = q.x; s[1] = q.y; s[2] = q.z; s[3] = q.w; }
			else for (int j = 0; j < cnt; ++j) s[j] = a.x[e + j];
			if (DDX) {
				float d[4] = {0.f, 0.f, 0.f, 0.f};
				if (whole) { const float4 q = *reinterpret_cast<const float4*>(a.data + e); d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w; }
				else for (int j = 0; j < cnt; ++j) d[j] = a.data[e + j];
				const float ga = a.ga[gi], gb = a.gb[gi];
#pragma unroll
				for (int j = 0; j < 4; ++j) { const float nv = (d[j] - m) / v; r[j] = (s[j] - ga - nv * gb) / v; }
			} else {
#pragma unroll
				for (int j = 0; j < 4; ++j) { const float t = (s[j] - m) / v; r[j] = t < 0.f ? 0.f : t; }
				if (a.drop) {
					if (whole) {   // (vec: the four decisions are one aligned 4-byte load)
						const uchar4 d = *reinterpret_cast<const uchar4*>(a.drop + e);
						if (d.x) r[0] = 0.f;
						if (d.y) r[1] = 0.f;
						if (d.z) r[2] = 0.f;
						if (d.w) r[3] = 0.f;
					} else
						for (int j = 0; j < cnt; ++j) if (a.drop[e + j]) r[j] = 0.f;
				}
			}
			if (a.out) {
				if (whole) *reinterpret_cast<float4*>(a.out + e) = make_float4(r[0], r[1], r[2], r[3]);
				else for (int j = 0; j < cnt; ++j) a.out[e + j] = r[j];
			}
		}
#pragma unroll
		for (int j = 0; j < 4; ++j) tile[c][x + j] = r[j];   // x + j <= 63; columns from xn up are never read
	}
	if (!a.dst.d) return;   // uniform over the launch
	__syncthreads();
	const int cq = threadIdx.x & 7, ch = c0 + cq * 8;
	if (ch >= a.dst.cp) return;
	uint16_t* drow = a.dst.d + (((size_t)b * a.dst.hp + a.dst.top + (size_t)y * a.dst.dilate) * a.dst.wp + a.dst.left) * a.dst.cp + ch;
	for (int px = threadIdx.x >> 3; px < xn; px += 32) {
		uint4 o;
		o.x = pack2(tile[cq * 8 + 0][px], tile[cq * 8 + 1][px]);
		o.y = pack2(tile[cq * 8 + 2][px], tile[cq * 8 + 3][px]);
		o.z = pack2(tile[cq * 8 + 4][px], tile[cq * 8 + 5][px]);
		o.w = pack2(tile[cq * 8 + 6][px], tile[cq * 8 + 7][px]);
		*reinterpret_cast<uint4*>(drow + (size_t)(x0 + px) * a.dst.dilate * a.dst.cp) = o;
	}
}

// ---- pure argument checks (no device is asked for) ---------------------------------------------------------------------------------------------------
bla_status check_norm_map(const char* who, int batch, int channels, int group_size, int h, int w, const void* out_f32, const bla_conv_bf16_map* dst) {
	BLA_REQUIRE(dst, BLA_ERR_INVALID, "%s: NULL dst", who);
	BLA_REQUIRE(dst->d || out_f32, BLA_ERR_INVALID, "%s: neither an fp32 output nor dst", who);
	BLA_REQUIRE(batch > 0 && channels > 0 && group_size > 0 && h > 0 && w > 0, BLA_ERR_INVALID, "%s: extent <= 0 (batch %d channels %d group_size %d h %d w %d)", who, batch,
	            channels, group_size, h, w);
	const long groups = ((long)channels + group_size - 1) / group_size;
	BLA_REQUIRE(batch <= 65535 && h <= 65535 && (long)batch * groups < (1L << 31) && (long)h * w < (1L << 31), BLA_ERR_INVALID, "%s: batch %d, h %d or %ld groups exceed the grid",
	            who, batch, h, (long)batch * groups);
	if (!dst->d) return BLA_OK;
	const bla_conv_bf16_map& m = *dst;
	BLA_REQUIRE(m.hp > 0 && m.wp > 0 && m.cp > 0, BLA_ERR_INVALID, "%s: dst has hp %d wp %d cp %d", who, m.hp, m.wp, m.cp);
	BLA_REQUIRE(m.cp == round8(channels), BLA_ERR_INVALID, "%s: dst.cp %d is not %d channels rounded up to 8", who, m.cp, channels);
	BLA_REQUIRE(aligned16(m.d), BLA_ERR_INVALID, "%s: dst is not 16-byte aligned", who);
	BLA_REQUIRE(m.top >= 0 && m.left >= 0 && m.dilate >= 1, BLA_ERR_INVALID, "%s: dst has top %d left %d dilate %d", who, m.top, m.left, m.dilate);
	BLA_REQUIRE((long)m.top + (long)(h - 1) * m.dilate < m.hp && (long)m.left + (long)(w - 1) * m.dilate < m.wp, BLA_ERR_INVALID,
	            "%s: the %d x %d tensor at (%d, %d), dilation %d, does not fit dst (%d x %d)", who, h, w, m.top, m.left, m.dilate, m.hp, m.wp);
	BLA_REQUIRE((long)batch * m.hp * m.wp * m.cp < (1L << 31), BLA_ERR_INVALID, "%s: dst holds %ld elements, 2^31 or more", who, (long)batch * m.hp * m.wp * m.cp);
	return BLA_OK;
}

template <bool DDX>
bla_status launch_apply(hipStream_t s, int batch, const ApplyArgs& a) {
	const long gx = (long)a.xtiles * ((a.channels + 63) / 64);   // (Cp <= the last tile's 64: the padding channels ride in the tile that holds channel C - 1)
	BLA_REQUIRE(gx < (1L << 31), BLA_ERR_INVALID, "group norm into a bf16 map: %d channels x %d columns exceed the grid", a.channels, a.w);
	hipLaunchKernelGGL(norm_bf16_apply_kernel<DDX>, dim3((unsigned)gx, a.h, batch), dim3(256), 0, s, a);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

}  // namespace
}  // namespace bla

using namespace bla;

extern "C" {

bla_status bla_group_norm_relu_bf16_map(void* stream, int batch, const float* d_in, int channels, int group_size, int h, int w, const unsigned char* d_drop, float* d_stdevs,
                                        float* d_means, float* d_out_f32, const bla_conv_bf16_map* dst) {
	const char* who = "bla_group_norm_relu_bf16_map";
	BLA_REQUIRE(d_in && d_means && d_stdevs, BLA_ERR_INVALID, "%s: NULL pointer", who);
	bla_status st = check_norm_map(who, batch, channels, group_size, h, w, d_out_f32, dst);
	if (st != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	hipStream_t s = pick_stream(stream);
	const int groups = (channels + group_size - 1) / group_size, hw = h * w;
	const StatArgs sa{d_in, nullptr, nullptr, nullptr, d_means, d_stdevs, channels, group_size, groups, hw, hw % 4 == 0 && aligned16(d_in)};
	hipLaunchKernelGGL(norm_bf16_stats_kernel<false>, dim3((unsigned)(batch * groups)), dim3(kStatThreads), 0, s, sa);
	BLA_HIP(hipGetLastError());
	const ApplyArgs a{d_in, nullptr, d_drop, d_means, d_stdevs, nullptr, nullptr, d_out_f32, *dst, channels, group_size, groups, h, w, (w + 63) / 64,
	                  w % 4 == 0 && aligned16(d_in) && aligned16(d_out_f32) && ((uintptr_t)d_drop & 3) == 0};
	return launch_apply<false>(s, batch, a);
}

bla_status bla_group_norm_ddx_bf16_map(void* stream, int batch, const float* d_source, const float* d_data, const float* d_means, const float* d_stdevs, int channels,
                                       int group_size, int h, int w, float* d_dest_f32, const bla_conv_bf16_map* dst) {
	const char* who = "bla_group_norm_ddx_bf16_map";
	BLA_REQUIRE(d_source && d_data && d_means && d_stdevs, BLA_ERR_INVALID, "%s: NULL pointer", who);
	bla_status st = check_norm_map(who, batch, channels, group_size, h, w, d_dest_f32, dst);
	if (st != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	hipStream_t s = pick_stream(stream);
	const int groups = (channels + group_size - 1) / group_size, hw = h * w;
	void* ws = nullptr;   // A and B, [batch][groups] each
	st = ensure_workspace((size_t)batch * groups * 2 * sizeof(float), &ws);
	if (st != BLA_OK) return st;
	float* ga = (float*)ws;
	float* gb = ga + (size_t)batch * groups;
	const StatArgs sa{d_source, d_data, d_means, d_stdevs, ga, gb, channels, group_size, groups, hw, hw % 4 == 0 && aligned16(d_source) && aligned16(d_data)};
	hipLaunchKernelGGL(norm_bf16_stats_kernel<true>, dim3((unsigned)(batch * groups)), dim3(kStatThreads), 0, s, sa);
	BLA_HIP(hipGetLastError());
	const ApplyArgs a{d_source, d_data, nullptr, d_means, d_stdevs, ga, gb, d_dest_f32, *dst, channels, group_size, groups, h, w, (w + 63) / 64,
	                  w % 4 == 0 && aligned16(d_source) && aligned16(d_data) && aligned16(d_dest_f32)};
	return launch_apply<true>(s, batch, a);
}

}  // extern "C"
