// bla_guidance.hip -- the class-conditional side of the diffusion U-Net (classifier-free guidance, Ho & Salimans 2022): a learned class embedding added
// to the time embedding, the label dropout that lets the same network learn the unconditional case, and the gradient of the embedding table.
//
// Not in the reference (its U-Net has no class input).  The table is [classes + 1][time_dim]; row `classes` is the learned null class.  The label
// dropout is the Bernoulli stream of bla_philox.h, so the rows an image used can be restated from (seed, offset) alone:
//   row_b = classes if bla_rand_bernoulli_u8(p_uncond, seed, offset)[b] else labels[b];   temb[b] += table[row_b]
// The table's gradient is the sum of the embedding gradients (bla_unet_embedding_grad_f32) of the images that used a row, in image order.
#include "bla_internal.h"
#include "bla_philox.h"
#include <cmath>
#include <vector>

using namespace bla;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBatch = 4096;   // the rows of a batch sit in LDS

unsigned grid_for(size_t work) {
	const size_t cap = 8 * (size_t)(ctx().num_cus > 0 ? ctx().num_cus : 256);
	size_t b = (work + kThreads - 1) / kThreads;
	return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// labels != NULL: row_b from the label and the Bernoulli draw (an out-of-range label gives row -1: nothing added), rows written; labels == NULL: rows holds them
__global__ void __launch_bounds__(kThreads) class_embedding_kernel(const float* __restrict__ table, int classes, const int* __restrict__ labels, int batch, int dim,
                                                                   unsigned long long thr, unsigned long long seed, unsigned long long offset, int* __restrict__ rows,
                                                                   float* __restrict__ temb) {
	__shared__ int rs[kMaxBatch];
	for (int b = threadIdx.x; b < batch; b += blockDim.x) {
		int r;
		if (labels) {
			const uint4 w = philox_block(seed, offset + (unsigned long long)b / 4, PHILOX_TAG_BERNOULLI);
			const int q = b % 4;
			const uint32_t u = q == 0 ? w.x : q == 1 ? w.y : q == 2 ? w.z : w.w;
			const int l = labels[b];
			r = (unsigned long long)u < thr ? classes : (l >= 0 && l <= classes ? l : -1);
			if (blockIdx.x == 0) rows[b] = r;
		} else {
			r = rows[b];
		}
		rs[b] = r;
	}
	__syncthreads();
	const size_t n = (size_t)batch * dim;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
		const int r = rs[i / dim];
		if (r >= 0 && r <= classes) temb[i] += table[(size_t)r * dim + i % dim];
	}
}

// gtable[k][t] = sum over the images b with rows[b] == k, in image order, of dtemb[b][t]; thread = (k, t)
__global__ void __launch_bounds__(kThreads) class_grad_kernel(const float* __restrict__ dtemb, const int* __restrict__ rows, int batch, int classes, int dim,
                                                              float* __restrict__ gtable) {
	__shared__ int rs[kMaxBatch];
	for (int b = threadIdx.x; b < batch; b += blockDim.x) rs[b] = rows[b];
	__syncthreads();
	const size_t n = (size_t)(classes + 1) * dim;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
		const int k = (int)(i / dim), t = (int)(i % dim);
		float acc = 0.f;
		for (int b = 0; b < batch; b++)
			if (rs[b] == k) acc += dtemb[(size_t)b * dim + t];
		gtable[i] = acc;
	}
}

}  // namespace

// labels the runtime does not know as device memory (plain or pinned host memory) are checked and mapped on the host
bool bla::host_pointer(const void* p) {
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return true; }
	return a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged && a.type != hipMemoryTypeUnified;
}

unsigned long long bla::bernoulli_threshold(float p) {
	const double t = std::floor((double)p * 4294967296.0);
	return (unsigned long long)(t < 0 ? 0.0 : (t > 4294967296.0 ? 4294967296.0 : t));
}

extern "C" {

bla_status bla_class_embedding_f32(void* stream, const float* d_table, int classes, const int* labels, int batch, int time_dim, float p_uncond,
                                   unsigned long long seed, unsigned long long offset, int* d_rows, float* d_temb) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(d_table && labels && d_rows && d_temb, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(classes >= 1 && batch >= 1 && batch <= kMaxBatch && time_dim >= 1, BLA_ERR_INVALID, "classes %d, batch %d (at most %d), time_dim %d", classes, batch,
	            kMaxBatch, time_dim);
	BLA_REQUIRE(!std::isnan(p_uncond), BLA_ERR_INVALID, "p_uncond is NaN");
	const unsigned long long thr = bernoulli_threshold(p_uncond);
	hipStream_t s = pick_stream(stream);
	const int* dev_labels = labels;
	if (host_pointer(labels)) {   // host labels: checked here, the rows formed here (the same Philox words) and handed to the kernel through d_rows
		std::vector<int> rows(batch);
		for (int b = 0; b < batch; b++) {
			BLA_REQUIRE(labels[b] >= 0 && labels[b] <= classes, BLA_ERR_INVALID, "label %d of image %d outside [0, %d]", labels[b], b, classes);
			const unsigned long long j = offset + (unsigned long long)b / 4;
			const uint4 w = philox4x32_10(make_uint4((uint32_t)j, (uint32_t)(j >> 32), PHILOX_TAG_BERNOULLI, 0u), (uint32_t)seed, (uint32_t)(seed >> 32));
			const int q = b % 4;
			const uint32_t u = q == 0 ? w.x : q == 1 ? w.y : q == 2 ? w.z : w.w;
			rows[b] = (unsigned long long)u < thr ? classes : labels[b];
		}
		BLA_HIP(hipMemcpyAsync(d_rows, rows.data(), (size_t)batch * sizeof(int), hipMemcpyHostToDevice, s));
		BLA_HIP(hipStreamSynchronize(s));   // (rows lives on this stack)
		dev_labels = nullptr;
	}
	hipLaunchKernelGGL(class_embedding_kernel, dim3(grid_for((size_t)batch * time_dim)), dim3(kThreads), 0, s, d_table, classes, dev_labels, batch, time_dim, thr, seed,
	                   offset, d_rows, d_temb);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_class_embedding_grad_f32(void* stream, const float* d_dtemb, const int* d_rows, int batch, int classes, int time_dim, float* d_gtable) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(d_dtemb && d_rows && d_gtable, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(classes >= 1 && batch >= 1 && batch <= kMaxBatch && time_dim >= 1, BLA_ERR_INVALID, "classes %d, batch %d (at most %d), time_dim %d", classes, batch,
	            kMaxBatch, time_dim);
	hipLaunchKernelGGL(class_grad_kernel, dim3(grid_for((size_t)(classes + 1) * time_dim)), dim3(kThreads), 0, pick_stream(stream), d_dtemb, d_rows, batch, classes,
	                   time_dim, d_gtable);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

}  // extern "C"
