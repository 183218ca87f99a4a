// bla_unet_model.hip -- the reference's U-Net (model/cifar_unet.c) assembled from the device-resident blocks of bla_unet.hip and bla_attention_*.hip:
// forward() (:1099-1166) and backward() (:1351-1436) for one image -- or for a batch of images at once (bla_unet_create_batched: every
// activation carries a leading image index, every image its own time embedding, the gradients are summed over the images: what a mini-batch
// of the reference's one-image-at-a-time loop accumulates) -- parameters and gradients in two flat buckets.
//
//   18 ResNet blocks (8 down, 2 mid, 8 up), 5 self-attention blocks (two at resolution 2 on the way down, one in the middle, two at
//   resolution 2 on the way up), 3 stride-2 down-convolutions, 3 nearest-neighbour up-samplings (each followed by a channel-changing
//   convolution only where the two resolutions' widths differ, :1131,1141,1151), 4 skip concatenations, output group-norm + ReLU + conv.
//
// The reference's own model is work in progress: its backward pass walks out of bounds, and several call sites hand the
// wrong buffers around.  This composition is the INTENDED network, block for block what the reference's functions compute when they are
// wired as their comments and the forward pass say:
//   * the second attention block of the third up-sampling stage has its own parameters and reads the second ResNet block's result
//     (as written :1150 calls the first block's parameters again and :1151 then reads an output nobody wrote);
//   * the data gradient of the three stride-2 convolutions is the stride-2 adjoint (as written :1412,1420,1430 pass stride 1 and _col2im
//     indexes out of bounds);
//   * a skip connection's gradient is ADDED to the gradient that arrives along the main path (as written :1424-1427 adds it first and
//     then lets _backward_attention overwrite the sum);
//   * convolution gradients land in the gradient bucket (as written :1203,1216 hand conv_ddx the parameters as the sink).
// Every block is pinned on its own against the reference's functions (tests/test_resnet.py, test_attention.py, test_conv_gpu.py,
// test_unet_glue.py); the composition is pinned against the same composition of the oracle's blocks (tests/test_unet_model.py).
// bla_unet_create_mixed(.., BLA_UNET_PRODUCTS_BF16) is the same composition with the ResNet blocks and the stand-alone convolutions on the bf16 stack:
// same buckets, same entries, one stream; pinned against a float64 restatement with the compositions' roundings (tests/test_unet_bf16_{host,gpu}.py).
//
// The wiring stands in ONE place, the step list kNetwork, and three walkers read it: bla_unet_create_heads forwards (parameter bucket, tensor names, dropout
// offsets; then every step's buffers and its input / output / skip pointers), bla_unet_forward_f32 forwards, unet_backward in reverse.  A change of topology is
// an edit of kNetwork (and of res[18] / att[5] / kEmbSplit if the number of blocks changes).  What the two product stacks do differently is one table of calls
// (Stack), chosen at create; which entries an attention block runs on is its stored route, decided in att_route (at create and by bla_unet_set_attention).
#include "bla_internal.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace bla;

namespace {
struct Tensor { size_t off, count; std::string name; };
struct Res {
	int cin, cout, h, w;
	size_t conv1, conv2, tw, tb, res;   // offsets in the buckets (res = SIZE_MAX when cin == cout)
	bla_resnet_params p;                // the same as addresses in the parameter bucket
	bla_resnet_grads g;                 // ... and in the gradient bucket
	bla_resnet_ws ws;
	float* result;
	ResnetPads pads = {nullptr, nullptr, false, false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // batched: zero-haloed padded copies of the two convolution inputs, filled by the norm kernels
	float* dtb = nullptr;                 // batched: per-image channel sums of the time-projection gradient [B][cout], kept until the pass's last launch
	size_t drop_off;                      // offset of this block's dropout decisions in the caller's mask
	bla_resnet_bf16_maps maps = {nullptr, nullptr, nullptr};   // bf16 products: the block's own padded channel-last maps (p1, p2: the gates, kept from forward to backward)
	ResnetBf16Prep prep16 = {};           // bf16 products: the block's kernel matrices in the model's table launches (all NULL: the block prepares them itself)
};
// one ResNet block's time-embedding projection (model/cifar_unet.c:1051-1052) and its gradients (:1191-1199); all 18 run as one launch each way
struct TimeJob { const float* w; const float* bias; float* tdense; const float* dtb; float* g_tw; float* g_tb; int cout; };
enum AttRoute { ROUTE_NONE, ROUTE_F32, ROUTE_BF16, ROUTE_ONLINE, ROUTE_F32_HEADS, ROUTE_ONLINE_HEADS, ROUTE_F32_ONLINE };   // the entries an attention block runs on (att_route)
struct Att {
	int c, h, w;
	AttRoute route;   // decided by att_route at create and at every bla_unet_set_attention
	size_t wq, wk, wv, wo, bias;
	bla_attention_ws fwd;
	size_t raw_floats, weights_floats;   // what fwd.scores_raw and fwd.weights hold (bla_unet_set_attention: a route needs its buffers)
	float* out;
};
struct Conv {
	int cin, cout, h, w, stride, k;       // h, w: INPUT size
	size_t kern;
	float* out;
	bool present;
	const float *prep_fwd = nullptr, *prep_bwd = nullptr;   // batched: the kernel matrix as the forward / data-gradient product reads it (KernelPrepJob outputs)
	const uint16_t *prep16_fwd = nullptr, *prep16_bwd = nullptr;   // bf16 products: the same from the bf16 table launches
};
constexpr size_t kNone = (size_t)-1;

// THE NETWORK, stated once: its steps in forward order.  index: into res[] / att[] / down[] / up[] (RESIZE: the up-sampling stage, CONCAT: the skip connection
// it reads); level: the resolution 0..3 of the step's output; tap: the step's output is also skip connection `tap` (-1: none); name: of its parameter tensors.
// A step reads the previous step's output -- the first one the model's input (in == NULL), the one behind a CONCAT the concatenation -- and an UP whose two
// widths are equal is absent: it passes its input on.  create fills in / out / skip (a resized map, a concatenation and the output ReLU live in `out` alone).
enum StepKind { RES, ATT, DOWN, RESIZE, UP, CONCAT, OUT_NORM, OUT_CONV };
struct Step { StepKind kind; int index, level, tap; const char* name; const float* in; float* out; const float* skip; };
const Step kNetwork[] = {
	{RES, 0, 0, -1, "down_1_resnet_1"}, {RES, 1, 0, 3, "down_1_resnet_2"}, {DOWN, 0, 1, -1, "down_1_conv_kernels"},
	{RES, 2, 1, -1, "down_2_resnet_1"}, {ATT, 0, 1, -1, "down_2_self_attention_1"}, {RES, 3, 1, 2, "down_2_resnet_2"}, {ATT, 1, 1, -1, "down_2_self_attention_2"},
	{DOWN, 1, 2, -1, "down_2_conv_kernels"},
	{RES, 4, 2, -1, "down_3_resnet_1"}, {RES, 5, 2, 1, "down_3_resnet_2"}, {DOWN, 2, 3, -1, "down_3_conv_kernels"},
	{RES, 6, 3, -1, "down_4_resnet_1"}, {RES, 7, 3, 0, "down_4_resnet_2"},
	{RES, 8, 3, -1, "mid_resnet_1"}, {ATT, 2, 3, -1, "mid_self_attention"}, {RES, 9, 3, -1, "mid_resnet_2"},
	{CONCAT, 0, 3, -1, nullptr}, {RES, 10, 3, -1, "up_1_resnet_1"}, {RES, 11, 3, -1, "up_1_resnet_2"}, {RESIZE, 0, 2, -1, nullptr}, {UP, 0, 2, -1, "up_1_conv_kernels"},
	{CONCAT, 1, 2, -1, nullptr}, {RES, 12, 2, -1, "up_2_resnet_1"}, {RES, 13, 2, -1, "up_2_resnet_2"}, {RESIZE, 1, 1, -1, nullptr}, {UP, 1, 1, -1, "up_2_conv_kernels"},
	{CONCAT, 2, 1, -1, nullptr}, {RES, 14, 1, -1, "up_3_resnet_1"}, {ATT, 3, 1, -1, "up_3_self_attention_1"}, {RES, 15, 1, -1, "up_3_resnet_2"},
	{ATT, 4, 1, -1, "up_3_self_attention_2"}, {RESIZE, 2, 0, -1, nullptr}, {UP, 2, 0, -1, "up_3_conv_kernels"},
	{CONCAT, 3, 0, -1, nullptr}, {RES, 16, 0, -1, "up_4_resnet_1"}, {RES, 17, 0, -1, "up_4_resnet_2"},
	{OUT_NORM, 0, 0, -1, nullptr}, {OUT_CONV, 0, 0, -1, "output_conv_kernels"},   // :1163-1165
};

// What differs between the two product stacks (fp32: bla_unet.hip / bla_conv.hip; bf16: bla_conv_bf16.hip), chosen once per model from its
// `products`: a block's buffers, the kernel-matrix tables of the two passes, a block and a stand-alone convolution each way.  Nothing else asks which stack it is.
struct Stack {
	bla_status (*alloc_block)(bla_unet*, Res&);
	bla_status (*plan_tables)(bla_unet*);
	bla_status (*block_forward)(bla_unet*, void* stream, Res&, const float* in, const float* temb, const unsigned char* drop);
	bla_status (*block_backward)(bla_unet*, void* stream, Res&, const float* g, const float* x, float* out);      // g: gradient of the result, out: of the input x
	bla_status (*conv_forward)(bla_unet*, void* stream, const Conv&, const float* in);
	bla_status (*conv_backward)(bla_unet*, void* stream, const Conv&, const float* g, const float* x, float* out);
};
constexpr size_t kGradPool = 48;   // side lane: the write-once gradient buffers of a backward pass
}  // namespace

struct bla_unet {
	bla_unet_config cfg;
	int batch = 1;
	int attention = BLA_UNET_ATTENTION_F32;   // BLA_UNET_ATTENTION_BF16: the attention blocks that qualify on bla_attention_{forward,backward}_batched_bf16; _BF16_ONLINE: on the online-softmax entries (3.29)
	int heads = 1;                          // bla_unet_create_heads: heads of width cfg.key_dim in every attention block
	int products = BLA_UNET_PRODUCTS_F32;   // BLA_UNET_PRODUCTS_BF16: the blocks and the stand-alone convolutions on the bf16 stack, one stream
	const Stack* stack = nullptr;           // the calls of `products`
	int H[4], W[4], max_cout = 1;           // the four resolutions; the widest block output
	std::vector<Step> steps;               // kNetwork with in / out / skip resolved against this model's buffers
	std::vector<Tensor> tensors;
	size_t count = 0, drop_count = 0;
	float *params = nullptr, *grads = nullptr;
	Res res[18];
	Att att[5];
	Conv down[3], up[3], outc;
	float *out_mu = nullptr, *out_sd = nullptr;                // the output norm's statistics (the resized maps, the concatenations and the output ReLU: their steps' `out`)
	unsigned char* zero_drop = nullptr;
	// backward
	float *ring[3] = {nullptr, nullptr, nullptr}, *gskip[4] = {nullptr, nullptr, nullptr, nullptr};   // the rotating gradient buffers; the skip connections' gradients
	TimeJob* time_jobs = nullptr;                // device, one per ResNet block (batch > 1)
	TimeJob* emb_jobs = nullptr;                 // device, one per ResNet block, every configuration: dtb = where the backward pass leaves the block's per-image
	                                             // channel sums (r.dtb: then this IS time_jobs; the fp32 single-image model: the block's time-bias gradient itself,
	                                             // a table of its own) -- read by bla_unet_embedding_grad_f32
	bool defer_time_grads = false;               // the blocks leave their per-image channel sums in r.dtb, time_grads_all_kernel ends the backward pass (time_jobs and: a batch, or bf16 products)
	bool have_grads = false;                    // a backward pass has run since the last forward pass
	float* g_res = nullptr;                                      // batched: the residual 1x1 convolutions' data gradient (largest block input)
	// batched, weight gradients on the context's side lane (BLA_UNET_SIDE=0: off): every gradient buffer of a backward pass is written ONCE (a pool instead of
	// three rotating buffers), every block has its own g_out_b -- what the lane reads stays intact until the pass's one join
	bool side = false;
	std::vector<float*> gpool;
	float* dy_pad[4] = {nullptr, nullptr, nullptr, nullptr};   // per resolution: padded gradient scratch of the blocks' first convolutions (halo zeroed once)
	KernelPrepJob *prep_fwd = nullptr, *prep_bwd = nullptr;   // device: every convolution's kernel matrix re-ordered / flipped in ONE launch per pass
	int n_prep_fwd = 0, n_prep_bwd = 0;
	size_t prep_max = 0;
	bla_conv_bf16_prep_job *prep16_fwd = nullptr, *prep16_bwd = nullptr;   // device, bf16 products: every bf16 kernel matrix of a pass in ONE launch
	int n_prep16_fwd = 0, n_prep16_bwd = 0;
	size_t prep16_max_fwd = 0, prep16_max_bwd = 0;                         // the largest job's 8-element chunks
	float *dtb = nullptr, *partials = nullptr;   // batched blocks: per-image time-bias sums [B][Cout], per-image attention weight gradients [B][C*d]
	bla_resnet_scratch sc = {};
	bla_attention_ws agrad = {};
	size_t agrad_raw = 0, agrad_weights = 0;   // floats of agrad.scores_raw and agrad.weights
	size_t bytes = 0;                          // the sum of what dalloc handed out (bla_unet_device_bytes)
	const float* last_x = nullptr; const float* last_temb = nullptr;   // the last forward pass's (the backward pass reads them)
	std::vector<void*> owned;
};

namespace {
// n elements of device memory that the model owns (freed by bla_unet_destroy)
template <typename T> bla_status dalloc(bla_unet* m, T** p, size_t n) {
	void* q = nullptr;
	BLA_HIP(hipMalloc(&q, (n ? n : 1) * sizeof(T)));
	m->owned.push_back(q);
	m->bytes += (n ? n : 1) * sizeof(T);
	*p = (T*)q;
	return BLA_OK;
}
template <typename T> bla_status dalloc_zeroed(bla_unet* m, T** p, size_t n) {
	bla_status st = dalloc(m, p, n);
	if (st) return st;
	BLA_HIP(hipMemsetAsync(*p, 0, n * sizeof(T), ctx().stream));
	return BLA_OK;
}
// a host table of jobs as a device table (none: *d stays NULL)
template <typename T> bla_status upload_table(bla_unet* m, const T* v, size_t n, T** d) {
	bla_status st = n ? dalloc(m, d, n) : BLA_OK;
	if (st || !n) return st;
	BLA_HIP(hipMemcpy(*d, v, n * sizeof(T), hipMemcpyHostToDevice));
	return BLA_OK;
}
size_t add_tensor(bla_unet* m, const std::string& name, size_t count) {
	size_t off = m->count;
	m->tensors.push_back(Tensor{off, count, name});
	m->count += (count + 3) / 4 * 4;    // every tensor 16-byte aligned inside the bucket
	return off;
}
void plan_res(bla_unet* m, Res& r, const std::string& name, int cin, int cout, int h, int w) {
	const int k = m->cfg.kernel, t = m->cfg.time_dim;
	r.cin = cin; r.cout = cout; r.h = h; r.w = w;
	r.conv1 = add_tensor(m, name + ".conv_1_kernels", (size_t)cout * cin * k * k);
	r.conv2 = add_tensor(m, name + ".conv_2_kernels", (size_t)cout * cout * k * k);
	r.tw = add_tensor(m, name + ".time_weights", (size_t)t * cout);
	r.tb = add_tensor(m, name + ".time_biases", (size_t)cout);
	r.res = cin != cout ? add_tensor(m, name + ".residual_conv_kernels", (size_t)cout * cin) : kNone;
	r.drop_off = m->drop_count;
	m->drop_count += (size_t)cout * h * w;
}
void plan_att(bla_unet* m, Att& a, const std::string& name, int c, int h, int w) {
	const int d = m->cfg.key_dim * m->heads;   // the block's width: the heads side by side
	a.c = c; a.h = h; a.w = w;
	a.wq = add_tensor(m, name + ".Q_proj", (size_t)c * d);
	a.wk = add_tensor(m, name + ".K_proj", (size_t)c * d);
	a.wv = add_tensor(m, name + ".V_proj", (size_t)c * d);
	a.wo = add_tensor(m, name + ".weights", (size_t)d * c);
	a.bias = add_tensor(m, name + ".biases", (size_t)c);
}
void plan_conv(bla_unet* m, Conv& c, const std::string& name, int cin, int cout, int h, int w, int stride, bool present = true) {
	c.cin = cin; c.cout = cout; c.h = h; c.w = w; c.stride = stride; c.k = m->cfg.kernel; c.present = present; c.out = nullptr;
	c.kern = present ? add_tensor(m, name, (size_t)cout * cin * c.k * c.k) : kNone;
}
// The second ReLU's output before dropout: the backward pass gates on the dropped form alone (dp = drop ? 0 : relu2 is zero wherever relu2 is), so a batched
// model whose norms run on the 16-byte kernels (rows of whole float4, a batch that folds into the channel count) does not store it
bool keep_relu2(const bla_unet* m, const Res& r) {
	const int gs = m->cfg.group_size;
	return !(m->batch > 1 && (r.h * r.w) % 4 == 0 && (r.cout % gs == 0 || r.cout < gs));
}
// a zero-filled padded channel-last bf16 map [B][hp][wp][round8(c)] in the layout bla_conv_bf16_layout states (the blocks write pixel positions only: the halo stays)
bla_status alloc_map(bla_unet* m, uint16_t** p, int c, int h, int w, bool data_gradient) {
	int hp, wp, top, left, dilate;
	bla_status st = bla_conv_bf16_layout(h, w, m->cfg.kernel, 1, data_gradient, &hp, &wp, &top, &left, &dilate);
	return st ? st : dalloc_zeroed(m, p, (size_t)m->batch * hp * wp * round8(c));
}
// bf16 products: relu1, relu2, dp, the fp32 padded copies and the fp32 prepared kernels have no reader; the three maps take their place.  Every block its own
// p1 / p2 (the gates of its backward pass) and its own q1.  The per-image channel sums (dtb) at every batch: the time gradients are always deferred here.
bla_status alloc_res_bf16(bla_unet* m, Res& r) {
	const size_t hw = (size_t)r.h * r.w * m->batch;
	const int gs = m->cfg.group_size, g1 = (r.cin + gs - 1) / gs * m->batch, g2 = (r.cout + gs - 1) / gs * m->batch;
	bla_status st;
	r.ws = bla_resnet_ws{};
	if ((st = dalloc(m, &r.ws.mu1, g1)) || (st = dalloc(m, &r.ws.sd1, g1)) || (st = dalloc(m, &r.ws.c1, r.cout * hw)) || (st = dalloc(m, &r.ws.tdense, (size_t)r.cout * m->batch)) ||
	    (st = dalloc(m, &r.ws.mu2, g2)) || (st = dalloc(m, &r.ws.sd2, g2)) || (st = dalloc(m, &r.ws.c2, r.cout * hw)) || (st = dalloc(m, &r.result, r.cout * hw)) ||
	    (st = dalloc(m, &r.dtb, (size_t)r.cout * m->batch)))
		return st;
	if (r.cin != r.cout && (st = dalloc(m, &r.ws.res, r.cout * hw))) return st;
	if ((st = alloc_map(m, &r.maps.p1, r.cin, r.h, r.w, false)) || (st = alloc_map(m, &r.maps.p2, r.cout, r.h, r.w, false)) || (st = alloc_map(m, &r.maps.q1, r.cout, r.h, r.w, true)))
		return st;
	return BLA_OK;
}
bla_status alloc_res(bla_unet* m, Res& r) {
	const size_t hw = (size_t)r.h * r.w * m->batch;   // (every buffer of the block: B times its single-image size)
	const int gs = m->cfg.group_size, g1 = (r.cin + gs - 1) / gs * m->batch, g2 = (r.cout + gs - 1) / gs * m->batch;
	bla_status st;
	if ((st = dalloc(m, &r.ws.mu1, g1)) || (st = dalloc(m, &r.ws.sd1, g1)) || (st = dalloc(m, &r.ws.relu1, r.cin * hw)) || (st = dalloc(m, &r.ws.c1, r.cout * hw)) ||
	    (st = dalloc(m, &r.ws.tdense, (size_t)r.cout * m->batch)) || (st = dalloc(m, &r.ws.mu2, g2)) || (st = dalloc(m, &r.ws.sd2, g2)) ||
	    (keep_relu2(m, r) ? (st = dalloc(m, &r.ws.relu2, r.cout * hw)) : (r.ws.relu2 = nullptr, BLA_OK)) ||
	    (st = dalloc(m, &r.ws.dp, r.cout * hw)) || (st = dalloc(m, &r.ws.c2, r.cout * hw)) || (st = dalloc(m, &r.result, r.cout * hw)))
		return st;
	r.ws.res = nullptr;
	if (r.cin != r.cout && (st = dalloc(m, &r.ws.res, r.cout * hw))) return st;
	if (m->batch == 1) return BLA_OK;
	if ((st = dalloc(m, &r.dtb, (size_t)r.cout * m->batch))) return st;
	if (r.cin != r.cout && r.cin > 4) {      // (one scratch for all blocks: they run one after the other)
		size_t widest = 0;
		for (int i = 0; i < 18; i++) if (m->res[i].cin != m->res[i].cout) widest = std::max(widest, (size_t)m->batch * m->res[i].cin * m->res[i].h * m->res[i].w);
		if (!m->g_res && (st = dalloc(m, &m->g_res, widest))) return st;
		r.pads.g_res = m->g_res;
	}
	// padded copies (conv_padded_layout): only where a tiled convolution will read them -- not for the 3-channel input of the first block (direct kernels)
	static const bool pads_on = [] { const char* e = getenv("BLA_UNET_PADS"); return !(e && e[0] == '0'); }();
	const PadLayout L = conv_padded_layout(r.h, r.w, m->cfg.kernel, 1);
	if (pads_on && L.plane > 0) {
		const size_t p1 = (size_t)m->batch * r.cin * L.plane, p2 = (size_t)m->batch * r.cout * L.plane;
		if (r.cin > 4 && (st = dalloc_zeroed(m, &r.pads.pad1, p1))) return st;
		if ((st = dalloc_zeroed(m, &r.pads.pad2, p2))) return st;
		// one scratch per resolution for the padded gradient in front of conv_1's data gradient (all blocks of a resolution share layout and halo)
		int res_i = 0;
		while (res_i < 3 && m->H[res_i] != r.h) res_i++;
		const size_t widest = (size_t)m->batch * std::max(std::max(m->cfg.dims[0], m->cfg.dims[1]), std::max(m->cfg.dims[2], m->cfg.dims[3])) * L.plane;
		if (!m->dy_pad[res_i] && (st = dalloc_zeroed(m, &m->dy_pad[res_i], widest))) return st;
		r.pads.dy_pad = m->dy_pad[res_i];
	}
	return BLA_OK;
}
// an attention workspace for sequences of s: q, k, v, attention [B][s][heads key_dim], then the two buffers whose floats the caller states (weights: 0 for none).
// One head: both B s s (scores and P; the bf16 entries keep row statistics at the head of scores_raw) under EVERY mode: a later switch must work (DESIGN 3.29
// "Open").  Several heads (3.31): scores_raw one float per (image, head, row), the online entries' statistics; P only in a block the fp32 heads entries apply to.
bla_status alloc_att_ws(bla_unet* m, bla_attention_ws& ws, size_t s, size_t scores_raw, size_t weights) {
	bla_status st;
	const size_t n = (size_t)m->batch * s * m->heads * m->cfg.key_dim;
	ws = bla_attention_ws{};
	if ((st = dalloc(m, &ws.q, n)) || (st = dalloc(m, &ws.k, n)) || (st = dalloc(m, &ws.v, n)) || (st = dalloc(m, &ws.attention, n)) ||
	    (st = dalloc(m, &ws.scores_raw, scores_raw)))
		return st;
	return weights ? dalloc(m, &ws.weights, weights) : BLA_OK;
}

// tdense[b][c] = sum_t temb[b][t] W[t][c] + bias[c] for every block at once: grid (block, 8 images, 64 channels); a workgroup = 64 channels x 4 quarters of
// the t range, the eight embedding rows in LDS, the quarters folded through LDS in quarter order (t ascending inside a quarter)
__global__ void __launch_bounds__(256) time_dense_all_kernel(const TimeJob* __restrict__ jobs, const float* __restrict__ temb, int batch, int tdim) {
	extern __shared__ float te[];             // [8][tdim], then [4][8][64] partial sums
	float* part = te + 8 * tdim;
	const TimeJob j = jobs[blockIdx.x];
	const int c0 = blockIdx.z * 64;
	if (c0 >= j.cout) return;                 // (whole workgroups: before any barrier)
	const int b0 = blockIdx.y * 8, nb = min(8, batch - b0);
	for (int e = threadIdx.x; e < 8 * tdim; e += 256) te[e] = e < nb * tdim ? temb[(size_t)b0 * tdim + e] : 0.f;
	__syncthreads();
	const int lane = threadIdx.x & 63, quarter = threadIdx.x >> 6, c = c0 + lane;
	const int per = (tdim + 3) / 4, t0 = quarter * per, t1 = min(tdim, t0 + per);
	float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
	if (c < j.cout)
#pragma unroll 8
		for (int t = t0; t < t1; t++) {      // (eight weight loads in flight: one by one this loop is 128 dependent round trips, 53 us)
			const float wv = j.w[(size_t)t * j.cout + c];
#pragma unroll
			for (int i = 0; i < 8; i++) acc[i] = fmaf(te[i * tdim + t], wv, acc[i]);
		}
#pragma unroll
	for (int i = 0; i < 8; i++) part[(quarter * 8 + i) * 64 + lane] = acc[i];
	__syncthreads();
	for (int e = threadIdx.x; e < 8 * 64; e += 256) {
		const int i = e >> 6, l = e & 63;
		if (i < nb && c0 + l < j.cout)
			j.tdense[(size_t)(b0 + i) * j.cout + c0 + l] = ((part[(0 * 8 + i) * 64 + l] + part[(1 * 8 + i) * 64 + l]) + (part[(2 * 8 + i) * 64 + l] + part[(3 * 8 + i) * 64 + l])) + j.bias[c0 + l];
	}
}
// g_tw[t][c] = sum_b temb[b][t] dtb[b][c], g_tb[c] = sum_b dtb[b][c] (images in order): grid (block, tdim / 8), thread = channel
__global__ void __launch_bounds__(256) time_grads_all_kernel(const TimeJob* __restrict__ jobs, const float* __restrict__ temb, int batch, int tdim) {
	const TimeJob j = jobs[blockIdx.x];
	const int t0 = blockIdx.y * 8, nt = min(8, tdim - t0);
	for (int c = threadIdx.x; c < j.cout; c += 256) {
		float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, sb = 0.f;
#pragma unroll 8
		for (int b = 0; b < batch; b++) {
			const float d = j.dtb[(size_t)b * j.cout + c];
			sb += d;
#pragma unroll
			for (int i = 0; i < 8; i++) acc[i] = fmaf(i < nt ? temb[(size_t)b * tdim + t0 + i] : 0.f, d, acc[i]);
		}
		for (int i = 0; i < nt; i++) j.g_tw[(size_t)(t0 + i) * j.cout + c] = acc[i];
		if (blockIdx.y == 0) j.g_tb[c] = sb;
	}
}
// dtemb[b][t] = sum_k sum_c W_k[t][c] dtb_k[b][c] -- the gradient of the time-embedding input, which feeds nothing but the 18 projections: grid (tdim / 8,
// batch / 8), a workgroup = 8 embedding rows x 8 images.  Wave w takes the blocks [kEmbSplit[w], kEmbSplit[w + 1]) in order, lane l the channels c = l mod 64
// of each, so every W_k row segment is read coalesced and once per tile of images; the 64 x 64 lane partials of each wave go through LDS and are summed in
// lane order, then the four waves' sums in wave order.  The order is fixed: bit-reproducible.
constexpr int kEmbSplit[5] = {0, 5, 9, 14, 18};
__global__ void __launch_bounds__(256) temb_grad_all_kernel(const TimeJob* __restrict__ jobs, int batch, int tdim, float* __restrict__ dtemb) {
	__shared__ float part[4][64][65];       // [wave][output = image * 8 + row][lane]
	__shared__ float wsum[4][64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int t0 = blockIdx.x * 8, nt = min(8, tdim - t0), b0 = blockIdx.y * 8, nb = min(8, batch - b0);
	float acc[8][8];                        // [image][row]
#pragma unroll
	for (int i = 0; i < 8; i++)
#pragma unroll
		for (int j = 0; j < 8; j++) acc[i][j] = 0.f;
	const int k1 = wave == 0 ? kEmbSplit[1] : wave == 1 ? kEmbSplit[2] : wave == 2 ? kEmbSplit[3] : kEmbSplit[4];
	for (int k = wave == 0 ? 0 : wave == 1 ? kEmbSplit[1] : wave == 2 ? kEmbSplit[2] : kEmbSplit[3]; k < k1; k++) {
		const TimeJob j = jobs[k];
#pragma unroll 2
		for (int c = lane; c < j.cout; c += 64) {
			float d[8], w[8];
#pragma unroll
			for (int i = 0; i < 8; i++) d[i] = i < nb ? j.dtb[(size_t)(b0 + i) * j.cout + c] : 0.f;
#pragma unroll
			for (int r = 0; r < 8; r++) w[r] = r < nt ? j.w[(size_t)(t0 + r) * j.cout + c] : 0.f;
#pragma unroll
			for (int i = 0; i < 8; i++)
#pragma unroll
				for (int r = 0; r < 8; r++) acc[i][r] = fmaf(w[r], d[i], acc[i][r]);
		}
	}
#pragma unroll
	for (int i = 0; i < 8; i++)
#pragma unroll
		for (int r = 0; r < 8; r++) part[wave][i * 8 + r][lane] = acc[i][r];
	__syncthreads();
	float s = 0.f;                          // thread (wave, lane): output `lane` of wave `wave`, its 64 lanes in order
	for (int l = 0; l < 64; l++) s += part[wave][lane][l];
	wsum[wave][lane] = s;
	__syncthreads();
	if (wave == 0) {
		const int i = lane >> 3, r = lane & 7;
		if (i < nb && r < nt) dtemb[(size_t)(b0 + i) * tdim + t0 + r] = ((wsum[0][lane] + wsum[1][lane]) + wsum[2][lane]) + wsum[3][lane];
	}
}
// del_Y = 2 (prediction - noise), model/cifar_unet.c:1353-1364
__global__ void __launch_bounds__(256) unet_loss_grad_kernel(const float* __restrict__ out, const float* __restrict__ noise, float* __restrict__ g, int n) {
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) g[i] = 2.f * (out[i] - noise[i]);
}
// _concat_skip, model/cifar_unet.c:1088-1097, per image: cat[b] = (a[b], skip[b]), both halves n floats
__global__ void __launch_bounds__(256) unet_concat_kernel(const float* __restrict__ a, const float* __restrict__ skip, float* __restrict__ cat, size_t n, size_t total) {
	for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
		const size_t b = e / (2 * n), r = e - b * 2 * n;
		cat[e] = r < n ? a[b * n + r] : skip[b * n + r - n];
	}
}
// the same 16 bytes at a time (n a multiple of 4)
__global__ void __launch_bounds__(256) unet_concat4_kernel(const float4* __restrict__ a, const float4* __restrict__ skip, float4* __restrict__ cat, size_t n4, size_t total4) {
	for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total4; e += (size_t)gridDim.x * blockDim.x) {
		const size_t b = e / (2 * n4), r = e - b * 2 * n4;
		cat[e] = r < n4 ? a[b * n4 + r] : skip[b * n4 + r - n4];
	}
}
__global__ void __launch_bounds__(256) unet_split4_kernel(const float4* __restrict__ g_cat, float4* __restrict__ g_main, float4* __restrict__ g_skip, size_t n4, size_t total4) {
	for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total4; e += (size_t)gridDim.x * blockDim.x) {
		const size_t b = e / (2 * n4), r = e - b * 2 * n4;
		const float4 v = g_cat[e];
		if (r < n4) g_main[b * n4 + r] = v; else g_skip[b * n4 + r - n4] = v;
	}
}
// _split_concat, :1339-1349, per image: the first half is the main path's gradient, the second the skip connection's
__global__ void __launch_bounds__(256) unet_split_kernel(const float* __restrict__ g_cat, float* __restrict__ g_main, float* __restrict__ g_skip, size_t n, size_t total) {
	for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
		const size_t b = e / (2 * n), r = e - b * 2 * n;
		const float v = g_cat[e];
		if (r < n) g_main[b * n + r] = v; else g_skip[b * n + r - n] = v;
	}
}
unsigned grid_of(size_t n) { size_t b = (n + 255) / 256; return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b)); }

// ---- the steps' calls -------------------------------------------------------------------------------------------------------------------------------------
Conv& conv_of(bla_unet* m, const Step& s) { return s.kind == DOWN ? m->down[s.index] : s.kind == UP ? m->up[s.index] : m->outc; }
// an absent step launches nothing either way and writes no gradient
bool step_runs(bla_unet* m, const Step& s) { return s.kind != UP || conv_of(m, s).present; }
bla_status block_forward_f32(bla_unet* m, void* stream, Res& r, const float* in, const float* temb, const unsigned char* drop) {
	const bla_unet_config& c = m->cfg;
	return resnet_forward_batched(stream, m->batch, in, temb, &r.p, drop, &r.ws, r.result, r.h, r.w, r.cin, r.cout, c.kernel, c.time_dim, c.group_size,
	                              m->time_jobs ? RESNET_TDENSE_READY : 0, m->batch > 1 ? &r.pads : nullptr);
}
bla_status block_forward_bf16(bla_unet* m, void* stream, Res& r, const float* in, const float* temb, const unsigned char* drop) {
	const bla_unet_config& c = m->cfg;
	return resnet_forward_bf16(stream, m->batch, in, temb, &r.p, drop, &r.ws, r.result, r.h, r.w, r.cin, r.cout, c.kernel, c.time_dim, c.group_size, &r.maps,
	                           m->time_jobs ? RESNET_TDENSE_READY : 0, &r.prep16);
}
bla_status block_backward_f32(bla_unet* m, void* stream, Res& r, const float* g, const float* x, float* out) {
	const bla_unet_config& c = m->cfg;
	const int B = m->batch;
	return resnet_backward_batched(stream, B, g, x, m->last_temb, &r.p, &r.ws, &r.g, &m->sc, B > 1 ? r.dtb : m->dtb, out, r.h, r.w, r.cin, r.cout, c.kernel, c.time_dim,
	                               c.group_size, (m->defer_time_grads ? RESNET_DEFER_TIME_GRADS : 0) | (m->side ? RESNET_WGRAD_SIDE : 0), B > 1 ? &r.pads : nullptr);
}
bla_status block_backward_bf16(bla_unet* m, void* stream, Res& r, const float* g, const float* x, float* out) {
	const bla_unet_config& c = m->cfg;   // (the channel sums go to r.dtb at every batch: bla_unet_embedding_grad_f32 reads them there)
	return resnet_backward_bf16(stream, m->batch, g, x, m->last_temb, &r.p, &r.ws, &r.g, &m->sc, r.dtb, out, r.h, r.w, r.cin, r.cout, c.kernel, c.time_dim, c.group_size,
	                            &r.maps, 0, m->defer_time_grads ? RESNET_DEFER_TIME_GRADS : 0, &r.prep16);
}
bla_status conv_forward_f32(bla_unet* m, void* stream, const Conv& k, const float* in) {
	return conv2d_forward_epilogue(stream, in, m->params + k.kern, k.out, k.h, k.w, k.k, k.cin, k.cout, k.stride, nullptr, nullptr, nullptr, m->batch, 0, nullptr, k.prep_fwd);
}
bla_status conv_forward_bf16(bla_unet* m, void* stream, const Conv& k, const float* in) {
	return conv2d_forward_as_bf16(stream, in, m->params + k.kern, k.out, m->batch, k.h, k.w, k.k, k.cin, k.cout, k.stride, nullptr, 0, k.prep16_fwd);
}
bla_status conv_backward_f32(bla_unet* m, void* stream, const Conv& k, const float* g, const float* x, float* out) {
	const float* kern = m->params + k.kern;
	float* g_kern = m->grads + k.kern;
	const int B = m->batch;
	if (m->side) {      // weight gradient on the side lane (g and x stay intact until the pass's join), data gradient here
		hipStream_t lane;
		bla_status st = side_lane_fork(pick_stream(stream), &lane);
		if (st) return st;
		st = conv2d_backward_batched(lane, g, x, kern, g_kern, nullptr, m->sc.flip, B, k.h, k.w, k.k, k.cin, k.cout, k.stride, nullptr, nullptr);
		side_lane_done();
		if (st) return st;
		g_kern = nullptr;
	}
	return conv2d_backward_batched(stream, g, x, kern, g_kern, out, m->sc.flip, B, k.h, k.w, k.k, k.cin, k.cout, k.stride, nullptr, k.prep_bwd);
}
bla_status conv_backward_bf16(bla_unet* m, void* stream, const Conv& k, const float* g, const float* x, float* out) {
	return conv2d_backward_gathered_as_bf16(stream, g, x, m->params + k.kern, m->grads + k.kern, out, m->batch, k.h, k.w, k.k, k.cin, k.cout, k.stride, 0, k.prep16_bwd);
}
// THE ROUTING RULE, stated once: the entries a block of c channels and s positions runs on under `mode`, with `heads` heads of width d.
//   one head:      the mode's bf16 entries where they apply to the shape, else fp32, which takes any shape (never ROUTE_NONE);
//   several heads: where both the fp32 heads entries (S <= 64) and the online ones apply, the mode chooses; else the one that applies, under EVERY mode -- a long
//                  block is bf16-online under both modes.  ROUTE_NONE: neither applies, so no mode can run the block (BLA_UNET_ATTENTION_BF16 has no heads).
//   BLA_UNET_ATTENTION_F32_ONLINE: a block with S > 64 runs the online fp32 entries, whatever the heads; every other block as under _F32.
AttRoute att_route(int mode, int heads, int c, int s, int d) {
	if (mode == BLA_UNET_ATTENTION_F32_ONLINE) {
		if (s > 64 && bla_attention_online_f32_applies(c, s, heads, d)) return ROUTE_F32_ONLINE;
		mode = BLA_UNET_ATTENTION_F32;
	}
	const bool online_mode = mode == BLA_UNET_ATTENTION_BF16_ONLINE;
	if (heads == 1)
		return online_mode && bla_attention_online_bf16_applies(c, s, d) ? ROUTE_ONLINE : mode == BLA_UNET_ATTENTION_BF16 && bla_attention_bf16_applies(c, s, d) ? ROUTE_BF16 : ROUTE_F32;
	const bool f32 = bla_attention_f32_heads_applies(c, s, heads, d), online = bla_attention_online_bf16_heads_applies(c, s, heads, d);
	if (f32 && online) return online_mode ? ROUTE_ONLINE_HEADS : ROUTE_F32_HEADS;
	return f32 ? ROUTE_F32_HEADS : online ? ROUTE_ONLINE_HEADS : ROUTE_NONE;
}
// floats of scores_raw and of weights that a route reads or writes, in the block's own workspace and in the shared gradient workspace (what create allocates
// for it and what bla_unet_set_attention asks a model to own): the materialising routes S x S, the online ones a float a row, the fp32 heads route P alone
struct AttNeeds { size_t raw, weights, grad_raw, grad_weights; };
AttNeeds att_needs(AttRoute r, size_t B, size_t heads, size_t s) {
	switch (r) {
	case ROUTE_F32: case ROUTE_BF16: return {B * s * s, B * s * s, B * s * s, B * s * s};
	case ROUTE_ONLINE: case ROUTE_ONLINE_HEADS: case ROUTE_F32_ONLINE: return {B * heads * s, 0, B * heads * s, 0};
	case ROUTE_F32_HEADS: return {0, B * heads * s * s, 0, 0};
	case ROUTE_NONE: break;
	}
	return {0, 0, 0, 0};
}
bla_status att_forward(bla_unet* m, void* stream, Att& a, const float* in) {
	const float* P = m->params;
	const int s = a.h * a.w, d = m->cfg.key_dim;
	switch (a.route) {
	case ROUTE_F32: case ROUTE_BF16: case ROUTE_ONLINE:
		return (a.route == ROUTE_F32 ? bla_attention_forward_batched_f32 : a.route == ROUTE_BF16 ? bla_attention_forward_batched_bf16 : bla_attention_forward_batched_online_bf16)(
			stream, m->batch, in, P + a.wq, P + a.wk, P + a.wv, P + a.wo, P + a.bias, &a.fwd, a.out, a.c, s, d);
	case ROUTE_F32_HEADS: case ROUTE_ONLINE_HEADS:
		return (a.route == ROUTE_F32_HEADS ? bla_attention_forward_batched_f32_heads : bla_attention_forward_batched_online_bf16_heads)(
			stream, m->batch, in, P + a.wq, P + a.wk, P + a.wv, P + a.wo, P + a.bias, &a.fwd, a.out, a.c, s, m->heads, d);
	case ROUTE_F32_ONLINE:
		return bla_attention_forward_batched_online_f32(stream, m->batch, in, P + a.wq, P + a.wk, P + a.wv, P + a.wo, P + a.bias, &a.fwd, a.out, a.c, s, m->heads, d);
	case ROUTE_NONE: break;   // (create refuses such a model)
	}
	set_error("attention block without a route");
	return BLA_ERR_INVALID;
}
bla_status att_backward(bla_unet* m, void* stream, Att& a, const float* g, const float* x, float* out) {
	const float* P = m->params; float* G = m->grads;
	const int s = a.h * a.w, d = m->cfg.key_dim;
	switch (a.route) {
	case ROUTE_F32:
		return bla_attention_backward_batched_f32(stream, m->batch, g, x, P + a.wq, P + a.wk, P + a.wv, P + a.wo, &a.fwd, &m->agrad, m->partials, G + a.wq, G + a.wk,
		                                          G + a.wv, G + a.wo, out, a.c, s, d, 0);
	case ROUTE_BF16: case ROUTE_ONLINE:
		return (a.route == ROUTE_BF16 ? bla_attention_backward_batched_bf16 : bla_attention_backward_batched_online_bf16)(
			stream, m->batch, g, x, P + a.wq, P + a.wk, P + a.wv, P + a.wo, &a.fwd, &m->agrad, m->partials, G + a.wq, G + a.wk, G + a.wv, G + a.wo, out, a.c, s, d);
	case ROUTE_F32_HEADS: case ROUTE_ONLINE_HEADS:
		return (a.route == ROUTE_F32_HEADS ? bla_attention_backward_batched_f32_heads : bla_attention_backward_batched_online_bf16_heads)(
			stream, m->batch, g, x, P + a.wq, P + a.wk, P + a.wv, P + a.wo, &a.fwd, &m->agrad, m->partials, G + a.wq, G + a.wk, G + a.wv, G + a.wo, out, a.c, s, m->heads, d);
	case ROUTE_F32_ONLINE:
		return bla_attention_backward_batched_online_f32(stream, m->batch, g, x, P + a.wq, P + a.wk, P + a.wv, P + a.wo, &a.fwd, &m->agrad, m->partials, G + a.wq, G + a.wk,
		                                                 G + a.wv, G + a.wo, out, a.c, s, m->heads, d);
	case ROUTE_NONE: break;
	}
	set_error("attention block without a route");
	return BLA_ERR_INVALID;
}
// floats per image of a map at the width and size of resolution `level`: a tapped output, one half of a concatenation
size_t level_floats(const bla_unet* m, int level) { return (size_t)m->cfg.dims[level] * m->H[level] * m->W[level]; }
// _concat_skip, model/cifar_unet.c:1088-1097: (the previous step's output, skip connection s.index) -> cat[s.index]
bla_status concat(bla_unet* m, hipStream_t stream, const Step& s) {
	const size_t n = level_floats(m, s.level), B = m->batch;
	if (n % 4 == 0 && ((uintptr_t)s.in | (uintptr_t)s.skip | (uintptr_t)s.out) % 16 == 0)
		hipLaunchKernelGGL(unet_concat4_kernel, dim3(grid_of(n / 2 * B)), dim3(256), 0, stream, (const float4*)s.in, (const float4*)s.skip, (float4*)s.out, n / 4, n / 2 * B);
	else hipLaunchKernelGGL(unet_concat_kernel, dim3(grid_of(2 * n * B)), dim3(256), 0, stream, s.in, s.skip, s.out, n, 2 * n * B);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}
// _split_concat, :1339-1349: the first half of a concatenation's gradient goes on along the main path, the second is skip connection s.index's
bla_status split(bla_unet* m, hipStream_t stream, const Step& s, const float* g_cat, float* g_main) {
	const size_t n = level_floats(m, s.level), B = m->batch;
	float* g_skip = m->gskip[s.index];
	if (n % 4 == 0 && ((uintptr_t)g_cat | (uintptr_t)g_main | (uintptr_t)g_skip) % 16 == 0)
		hipLaunchKernelGGL(unet_split4_kernel, dim3(grid_of(n / 2 * B)), dim3(256), 0, stream, (const float4*)g_cat, (float4*)g_main, (float4*)g_skip, n / 4, n / 2 * B);
	else hipLaunchKernelGGL(unet_split_kernel, dim3(grid_of(2 * n * B)), dim3(256), 0, stream, g_cat, g_main, g_skip, n, 2 * n * B);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}
// gradient buffers one backward pass writes: the loss seed, then one per step that runs -- but the first, whose input gradient nobody consumes
size_t backward_writes(bla_unet* m) { return 1 + std::count_if(m->steps.begin() + 1, m->steps.end(), [&](const Step& s) { return step_runs(m, s); }); }

// ---- the kernel-matrix tables of the two passes -----------------------------------------------------------------------------------------------------------
// fp32, batch > 1: one launch at the head of forward() and one at the head of backward() put every convolution's kernels into the form its product reads (window
// order, flipped): 49 five-microsecond launches per pass become 2.  The parameters do not change inside a pass, so the prepared copies are valid for it.
bla_status plan_tables_f32(bla_unet* m) {
	std::vector<KernelPrepJob> jf, jb;
	auto add = [&](size_t kern_off, int h, int w, int k, int cin, int cout, bool want_dgrad, const float** pf, const float** pb) -> bla_status {
		const size_t n = (size_t)cout * cin * k * k;
		const int mf = conv_kernel_prep_mode(m->batch, h, w, k, cin, cout, 1, false), mb = want_dgrad ? conv_kernel_prep_mode(m->batch, h, w, k, cin, cout, 1, true) : 0;
		for (int which = 0; which < 2; which++) {
			const int mode = which ? mb : mf;
			if (!mode) continue;
			float* dst;
			bla_status st = dalloc(m, &dst, n);
			if (st) return st;
			(which ? jb : jf).push_back(KernelPrepJob{m->params + kern_off, dst, cout, cin, k, mode});
			*(which ? pb : pf) = dst;
			m->prep_max = std::max(m->prep_max, n);
		}
		return BLA_OK;
	};
	bla_status st;
	for (int i = 0; i < 18; i++) {
		Res& r = m->res[i];
		if ((st = add(r.conv1, r.h, r.w, m->cfg.kernel, r.cin, r.cout, i != 0, &r.pads.k1_fwd, &r.pads.k1_bwd)) ||     // (block 0 forms no gradient of the image)
		    (st = add(r.conv2, r.h, r.w, m->cfg.kernel, r.cout, r.cout, true, &r.pads.k2_fwd, &r.pads.k2_bwd)))
			return st;
	}
	for (Conv& u : m->up)
		if (u.present && (st = add(u.kern, u.h, u.w, u.k, u.cin, u.cout, true, &u.prep_fwd, &u.prep_bwd))) return st;
	m->n_prep_fwd = (int)jf.size(); m->n_prep_bwd = (int)jb.size();
	if ((st = upload_table(m, jf.data(), jf.size(), &m->prep_fwd))) return st;
	return upload_table(m, jb.data(), jb.size(), &m->prep_bwd);
}
// bf16: one table launch at the head of each pass writes every bf16 kernel matrix of that pass into a matrix the model owns: the forward set is
// every convolution, the data-gradient set the same minus block 0's conv1 (nothing consumes the gradient of the image; its residual 1 x 1 likewise).
// BLA_UNET_BF16_PREP=0, read HERE at every create call: no tables, every composition prepares its own matrix in the workspace -- the same bits.
bla_status plan_tables_bf16(bla_unet* m) {
	const char* e = getenv("BLA_UNET_BF16_PREP");
	if (e && e[0] == '0') return BLA_OK;
	std::vector<bla_conv_bf16_prep_job> jf, jb;
	auto add = [&](size_t kern_off, int k, int cin, int cout, bool dgrad, const uint16_t** dst_out) -> bla_status {
		const int rows = dgrad ? cin : cout, ip = round8(dgrad ? cout : cin);
		const size_t chunks = (size_t)rows * k * k * (ip / 8);
		uint16_t* q = nullptr;
		bla_status st = dalloc(m, &q, chunks * 8);      // (hipMalloc: 16-byte aligned)
		if (st) return st;
		(dgrad ? jb : jf).push_back(bla_conv_bf16_prep_job{m->params + kern_off, q, cout, cin, k, dgrad ? 1 : 0});
		size_t& mx = dgrad ? m->prep16_max_bwd : m->prep16_max_fwd;
		mx = std::max(mx, chunks);
		*dst_out = q;
		return BLA_OK;
	};
	bla_status st;
	const int k = m->cfg.kernel;
	for (int i = 0; i < 18; i++) {
		Res& r = m->res[i];
		if ((st = add(r.conv1, k, r.cin, r.cout, false, &r.prep16.k1_fwd)) || (st = add(r.conv2, k, r.cout, r.cout, false, &r.prep16.k2_fwd)) ||
		    (st = add(r.conv2, k, r.cout, r.cout, true, &r.prep16.k2_bwd)))
			return st;
		if (i != 0 && (st = add(r.conv1, k, r.cin, r.cout, true, &r.prep16.k1_bwd))) return st;
		if (r.res != kNone && ((st = add(r.res, 1, r.cin, r.cout, false, &r.prep16.res_fwd)) || (i != 0 && (st = add(r.res, 1, r.cin, r.cout, true, &r.prep16.res_bwd)))))
			return st;
	}
	auto add_conv = [&](Conv& c) -> bla_status {
		if (!c.present) return BLA_OK;
		bla_status s2 = add(c.kern, c.k, c.cin, c.cout, false, &c.prep16_fwd);
		return s2 ? s2 : add(c.kern, c.k, c.cin, c.cout, true, &c.prep16_bwd);
	};
	for (int i = 0; i < 3; i++) if ((st = add_conv(m->down[i])) || (st = add_conv(m->up[i]))) return st;
	if ((st = add_conv(m->outc))) return st;
	m->n_prep16_fwd = (int)jf.size(); m->n_prep16_bwd = (int)jb.size();
	if ((st = upload_table(m, jf.data(), jf.size(), &m->prep16_fwd))) return st;
	return upload_table(m, jb.data(), jb.size(), &m->prep16_bwd);
}
const Stack kStackF32 = {alloc_res, plan_tables_f32, block_forward_f32, block_backward_f32, conv_forward_f32, conv_backward_f32};
const Stack kStackBf16 = {alloc_res_bf16, plan_tables_bf16, block_forward_bf16, block_backward_bf16, conv_forward_bf16, conv_backward_bf16};
}  // namespace

const bla_unet_config* bla::unet_config(const bla_unet* m) { return &m->cfg; }

extern "C" {

bla_status bla_unet_create(bla_unet** out, const bla_unet_config* cfg) { return bla_unet_create_batched(out, cfg, 1); }

bla_status bla_unet_create_batched(bla_unet** out, const bla_unet_config* cfg, int batch) { return bla_unet_create_mixed(out, cfg, batch, BLA_UNET_PRODUCTS_F32); }

int bla_unet_products(const bla_unet* m) { return m ? m->products : BLA_UNET_PRODUCTS_F32; }

int bla_unet_attention(const bla_unet* m) { return m ? m->attention : BLA_UNET_ATTENTION_F32; }

int bla_unet_heads(const bla_unet* m) { return m ? m->heads : 1; }

bla_status bla_unet_set_attention(bla_unet* m, int mode) {
	BLA_REQUIRE(mode == BLA_UNET_ATTENTION_F32 || mode == BLA_UNET_ATTENTION_BF16 || mode == BLA_UNET_ATTENTION_BF16_ONLINE || mode == BLA_UNET_ATTENTION_F32_ONLINE,
	            BLA_ERR_INVALID, "bla_unet_set_attention: mode %d (BLA_UNET_ATTENTION_F32, _BF16, _BF16_ONLINE or _F32_ONLINE)", mode);
	BLA_REQUIRE(m, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(m->heads == 1 || mode != BLA_UNET_ATTENTION_BF16, BLA_ERR_INVALID,
	            "bla_unet_set_attention: BLA_UNET_ATTENTION_BF16 on a model with %d heads (the materialising bf16 block has none)", m->heads);
	// every block needs a route under the new mode, and the buffers of that route: a model of the older create entries owns them under every mode accepted
	// above; one created in BLA_UNET_ATTENTION_F32_ONLINE (bla_unet_create_attention) may have neither
	AttRoute routes[5];
	for (int i = 0; i < 5; i++) {
		const Att& a = m->att[i];
		const size_t s = (size_t)a.h * a.w;
		routes[i] = att_route(mode, m->heads, a.c, (int)s, m->cfg.key_dim);
		const AttNeeds n = att_needs(routes[i], (size_t)m->batch, (size_t)m->heads, s);
		BLA_REQUIRE(routes[i] != ROUTE_NONE, BLA_ERR_INVALID, "bla_unet_set_attention: mode %d has no path for the block C=%d S=%zu heads=%d d=%d", mode, a.c, s, m->heads,
		            m->cfg.key_dim);
		BLA_REQUIRE(n.raw <= a.raw_floats && n.weights <= a.weights_floats && n.grad_raw <= m->agrad_raw && n.grad_weights <= m->agrad_weights, BLA_ERR_INVALID,
		            "bla_unet_set_attention: mode %d needs S x S buffers for the block C=%d S=%zu that this model was created without", mode, a.c, s);
	}
	m->attention = mode;
	for (int i = 0; i < 5; i++) m->att[i].route = routes[i];
	return BLA_OK;
}

bla_status bla_unet_create_mixed(bla_unet** out, const bla_unet_config* cfg, int batch, int products) { return bla_unet_create_heads(out, cfg, batch, products, 1); }

namespace {
bla_status create_model(bla_unet** out, const bla_unet_config* cfg, int batch, int products, int heads, int attention);
}
bla_status bla_unet_create_heads(bla_unet** out, const bla_unet_config* cfg, int batch, int products, int heads) {
	return create_model(out, cfg, batch, products, heads, BLA_UNET_ATTENTION_F32);
}

bla_status bla_unet_create_attention(bla_unet** out, const bla_unet_config* cfg, int batch, int products, int heads, int attention) {
	BLA_REQUIRE(attention == BLA_UNET_ATTENTION_F32 || attention == BLA_UNET_ATTENTION_BF16 || attention == BLA_UNET_ATTENTION_BF16_ONLINE ||
	            attention == BLA_UNET_ATTENTION_F32_ONLINE, BLA_ERR_INVALID, "bla_unet_create_attention: mode %d (BLA_UNET_ATTENTION_F32, _BF16, _BF16_ONLINE or _F32_ONLINE)",
	            attention);
	if (attention == BLA_UNET_ATTENTION_F32_ONLINE) return create_model(out, cfg, batch, products, heads, attention);
	bla_unet* m = nullptr;   // the other modes: bla_unet_create_heads, then the switch -- the same refusals, bits and bytes
	bla_status st = create_model(&m, cfg, batch, products, heads, BLA_UNET_ATTENTION_F32);
	if (st) return st;
	if ((st = bla_unet_set_attention(m, attention))) { (void)bla_unet_destroy(m); return st; }
	*out = m;
	return BLA_OK;
}

size_t bla_unet_device_bytes(const bla_unet* m) { return m ? m->bytes : 0; }

}  // extern "C"

namespace {
// attention == BLA_UNET_ATTENTION_F32: a model that every mode can run (bla_unet_create_heads: a block no multi-head path takes is refused, one head keeps its
// S x S buffers).  BLA_UNET_ATTENTION_F32_ONLINE: the model in that mode, every block's buffers those of its route.
bla_status create_model(bla_unet** out, const bla_unet_config* cfg, int batch, int products, int heads, int attention) {
	const bool in_mode = attention == BLA_UNET_ATTENTION_F32_ONLINE;
	BLA_REQUIRE(products == BLA_UNET_PRODUCTS_F32 || products == BLA_UNET_PRODUCTS_BF16, BLA_ERR_INVALID, "bla_unet_create_mixed: products %d (BLA_UNET_PRODUCTS_F32 or _BF16)", products);
	const bool bf16 = products == BLA_UNET_PRODUCTS_BF16;
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(out && cfg, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(batch >= 1 && batch <= 4096, BLA_ERR_INVALID, "batch %d", batch);
	BLA_REQUIRE(cfg->image_h > 0 && cfg->image_w > 0 && cfg->in_channels > 0 && cfg->time_dim > 0 && cfg->kernel > 0 && cfg->group_size > 0 && cfg->key_dim > 0 &&
	            cfg->dims[0] > 0 && cfg->dims[1] > 0 && cfg->dims[2] > 0 && cfg->dims[3] > 0, BLA_ERR_INVALID, "bad U-Net configuration");
	BLA_REQUIRE(cfg->image_h % 8 == 0 && cfg->image_w % 8 == 0, BLA_ERR_INVALID, "image size must be a multiple of 8 (three halvings, each undone by a x2 up-sampling)");
	BLA_REQUIRE(heads >= 1 && (heads == 1 || heads <= 256 / cfg->key_dim), BLA_ERR_INVALID, "bla_unet_create_heads: %d heads of width %d (heads >= 1, heads key_dim <= 256)",
	            heads, cfg->key_dim);
	bla_unet* m = new bla_unet();
	m->cfg = *cfg;
	m->batch = batch;
	m->heads = heads;
	m->attention = attention;
	m->products = products;
	m->stack = bf16 ? &kStackBf16 : &kStackF32;
	const size_t B = (size_t)batch;
	const int* D = cfg->dims;
	m->H[0] = cfg->image_h; m->W[0] = cfg->image_w;
	for (int i = 1; i < 4; i++) { m->H[i] = (m->H[i - 1] + 1) / 2; m->W[i] = (m->W[i - 1] + 1) / 2; }   // RESOLUTION_n_HEIGHT, :39-46
	const int* H = m->H; const int* W = m->W;
	// the parameter bucket, the tensor names and the dropout offsets: the steps in forward order, `ch` the channels that arrive at each
	m->steps.assign(std::begin(kNetwork), std::end(kNetwork));
	int ch = cfg->in_channels;
	for (const Step& s : m->steps) {
		const int l = s.level;
		switch (s.kind) {
		case RES: plan_res(m, m->res[s.index], s.name, ch, D[l], H[l], W[l]); ch = D[l]; break;
		case ATT: plan_att(m, m->att[s.index], s.name, ch, H[l], W[l]); break;
		case DOWN: plan_conv(m, m->down[s.index], s.name, ch, D[l], H[l - 1], W[l - 1], 2); ch = D[l]; break;
		case UP: plan_conv(m, m->up[s.index], s.name, ch, D[l], H[l], W[l], 1, ch != D[l]); ch = D[l]; break;   // (:1131,1141,1151: only where the widths differ)
		case CONCAT: ch *= 2; break;
		case OUT_CONV: plan_conv(m, m->outc, s.name, ch, cfg->in_channels, H[l], W[l], 1); break;
		case RESIZE: case OUT_NORM: break;
		}
	}

	auto fail = [&](bla_status s) { (void)bla_unet_destroy(m); return s; };
	for (Att& a : m->att)   // every block's route under the default mode; ROUTE_NONE: under no mode (several heads, neither multi-head path) -- before anything is allocated
		if ((a.route = att_route(m->attention, heads, a.c, a.h * a.w, cfg->key_dim)) == ROUTE_NONE) {
			set_error("bla_unet_create_heads: no multi-head attention path for C=%d S=%d heads=%d d=%d (fp32: S <= 64; online bf16: S %% 32 == 0, d %% 8 == 0, C %% 8 == 0)",
			          a.c, a.h * a.w, heads, cfg->key_dim);
			return fail(BLA_ERR_INVALID);
		}
	if ((st = dalloc_zeroed(m, &m->params, m->count)) || (st = dalloc_zeroed(m, &m->grads, m->count))) return fail(st);
	size_t max_act = 0, max_s = 0, max_flip = 0, max_cout_hw = 0, max_cin_hw = 0, max_cd = 1;
	for (Res& r : m->res) {
		if ((st = m->stack->alloc_block(m, r))) return fail(st);
		const float* P = m->params; float* G = m->grads;
		r.p = {P + r.conv1, P + r.conv2, P + r.tw, P + r.tb, r.res != kNone ? P + r.res : nullptr};
		r.g = {G + r.conv1, G + r.conv2, G + r.tw, G + r.tb, r.res != kNone ? G + r.res : nullptr};
		const size_t hw = (size_t)r.h * r.w * B;
		max_act = std::max(max_act, (size_t)std::max(r.cin, r.cout) * hw);
		max_cout_hw = std::max(max_cout_hw, r.cout * hw); max_cin_hw = std::max(max_cin_hw, r.cin * hw); m->max_cout = std::max(m->max_cout, r.cout);
		max_flip = std::max(max_flip, (size_t)r.cout * std::max(r.cin, r.cout) * cfg->kernel * cfg->kernel);
	}
	// the other steps' buffers, and every step's input, output and skip: a step reads what the step before it wrote
	float* prev = nullptr;   // the model's input
	const bool one_head = heads == 1;   // the attention workspaces (alloc_att_ws): one head keeps S x S scores and P, several one float a row and P where fp32 runs
	for (Step& s : m->steps) {
		const int l = s.level;
		const size_t n = B * level_floats(m, l);   // a map of the level's own width
		s.in = prev;
		switch (s.kind) {
		case RES: s.out = m->res[s.index].result; break;
		case ATT: {
			Att& a = m->att[s.index];
			const size_t sp = (size_t)a.h * a.w;
			// (under the default mode ROUTE_F32_HEADS is exactly "the fp32 heads entries apply": those blocks own P, whatever the mode turns to)
			const AttNeeds need = att_needs(a.route, B, heads, sp);
			a.raw_floats = in_mode ? need.raw : B * heads * sp * (one_head ? sp : 1);
			a.weights_floats = in_mode ? need.weights : one_head || a.route == ROUTE_F32_HEADS ? B * heads * sp * sp : 0;
			m->agrad_raw = std::max(m->agrad_raw, need.grad_raw); m->agrad_weights = std::max(m->agrad_weights, need.grad_weights);   // (in_mode: the largest block that still materialises)
			if ((st = alloc_att_ws(m, a.fwd, sp, a.raw_floats, a.weights_floats)) || (st = dalloc(m, &a.out, B * a.c * sp)))
				return fail(st);
			max_s = std::max(max_s, sp); max_cd = std::max(max_cd, (size_t)a.c * cfg->key_dim * heads);
			s.out = a.out;
			break;
		}
		case DOWN: case UP: case OUT_CONV: {
			Conv& k = conv_of(m, s);
			if (k.present && (st = dalloc(m, &k.out, B * k.cout * H[l] * W[l]))) return fail(st);
			if (k.present) max_flip = std::max(max_flip, (size_t)k.cout * k.cin * k.k * k.k);
			s.out = k.present ? k.out : prev;   // an absent up-convolution passes the resized map on
			break;
		}
		case RESIZE:   // (as wide as the input of the up-convolution behind it)
			if ((st = dalloc(m, &s.out, B * m->up[s.index].cin * H[l] * W[l]))) return fail(st);
			max_act = std::max(max_act, B * m->up[s.index].cin * H[l] * W[l]);
			break;
		case CONCAT:
			if ((st = dalloc(m, &s.out, 2 * n)) || (st = dalloc(m, &m->gskip[s.index], n))) return fail(st);
			max_act = std::max(max_act, 2 * n);
			for (const Step& t : m->steps) if (t.tap == s.index) s.skip = t.out;   // (tapped further up: resolved already)
			break;
		case OUT_NORM: {
			const int groups = (D[l] + cfg->group_size - 1) / cfg->group_size * batch;
			if ((st = dalloc(m, &s.out, n)) || (st = dalloc(m, &m->out_mu, groups)) || (st = dalloc(m, &m->out_sd, groups))) return fail(st);
			break;
		}
		}
		prev = s.out;
	}
	static const bool side_on = [] { const char* e = getenv("BLA_UNET_SIDE"); return !(e && e[0] == '0'); }();
	m->side = side_on && !bf16 && batch > 1 && kGradPool * max_act * sizeof(float) <= ((size_t)16 << 30);   // (the write-once pool: at most 16 GiB of it -- beyond that, one stream and three rotating buffers; bf16 products: one stream)
	if (m->side) {
		if (backward_writes(m) > kGradPool) {   // a buffer taken twice in a pass would be overwritten under the side lane's reads
			set_error("bla_unet_create: a backward pass writes %zu gradient buffers, the side lane's pool holds %zu", backward_writes(m), kGradPool);
			return fail(BLA_ERR_INVALID);
		}
		for (size_t i = 0; i < kGradPool; i++) { float* q; if ((st = dalloc(m, &q, max_act))) return fail(st); m->gpool.push_back(q); }
		for (Res& r : m->res) if ((st = dalloc(m, &r.pads.g_out_b, (size_t)r.cout * r.h * r.w * B))) return fail(st);
	}
	if (!in_mode) { m->agrad_raw = B * heads * max_s * (one_head ? max_s : 1); m->agrad_weights = one_head ? B * max_s * max_s : 0; }
	if ((st = dalloc(m, &m->ring[0], max_act)) || (st = dalloc(m, &m->ring[1], max_act)) || (st = dalloc(m, &m->ring[2], max_act)) || (st = dalloc(m, &m->sc.g_out_a, max_cout_hw)) ||
	    (st = dalloc(m, &m->sc.g_out_b, max_cout_hw)) || (st = dalloc(m, &m->sc.g_in, max_cin_hw)) || (st = dalloc(m, &m->sc.flip, max_flip)) ||
	    (st = alloc_att_ws(m, m->agrad, max_s, m->agrad_raw, m->agrad_weights)) || (st = dalloc(m, &m->dtb, B * m->max_cout)) || (st = dalloc(m, &m->partials, B * 4 * max_cd)))   // (4 C d an image: the bf16 attention entries keep all four weight-gradient partials)
		return fail(st);
	if ((st = dalloc_zeroed(m, &m->zero_drop, B * m->drop_count))) return fail(st);
	{   // the 18 time-embedding projections (and, for a batch, their gradients) as one launch each way (eight embedding rows in LDS), and the embedding gradient's
		// table (every configuration): the jobs' addresses are fixed from here on.  One table serves both wherever the backward pass leaves the per-image channel
		// sums in r.dtb; the fp32 single-image model leaves them in the time-bias gradient (a single image's channel sums ARE that gradient)
		TimeJob jobs[18];
		for (int i = 0; i < 18; i++) {
			const Res& r = m->res[i];
			jobs[i] = TimeJob{r.p.time_w, r.p.time_b, r.ws.tdense, r.dtb, r.g.time_w, r.g.time_b, r.cout};
		}
		if (cfg->time_dim <= 1024 && (st = upload_table(m, jobs, 18, &m->time_jobs))) return fail(st);
		const bool sums_in_dtb = batch > 1 || bf16;
		m->defer_time_grads = sums_in_dtb && m->time_jobs;
		m->emb_jobs = m->time_jobs;
		if (!sums_in_dtb) for (int i = 0; i < 18; i++) jobs[i].dtb = m->res[i].g.time_b;
		if ((!sums_in_dtb || !m->time_jobs) && (st = upload_table(m, jobs, 18, &m->emb_jobs))) return fail(st);
	}
	static const bool prep_on = [] { const char* e = getenv("BLA_UNET_PREP"); return !(e && e[0] == '0'); }();
	if ((bf16 || (batch > 1 && prep_on)) && (st = m->stack->plan_tables(m))) return fail(st);
	BLA_HIP(hipStreamSynchronize(ctx().stream));
	*out = m;
	return BLA_OK;
}
}  // namespace

extern "C" {

bla_status bla_unet_destroy(bla_unet* m) {
	if (!m) return BLA_OK;
	(void)hipDeviceSynchronize();
	for (void* p : m->owned) (void)hipFree(p);
	delete m;
	return BLA_OK;
}

size_t bla_unet_param_count(const bla_unet* m) { return m ? m->count : 0; }
float* bla_unet_params(bla_unet* m) { return m ? m->params : nullptr; }
float* bla_unet_grads(bla_unet* m) { return m ? m->grads : nullptr; }
float* bla_unet_output(bla_unet* m) { return m ? m->outc.out : nullptr; }
size_t bla_unet_dropout_count(const bla_unet* m) { return m ? m->drop_count * m->batch : 0; }
int bla_unet_batch(const bla_unet* m) { return m ? m->batch : 0; }
int bla_unet_tensor_count(const bla_unet* m) { return m ? (int)m->tensors.size() : 0; }

bla_status bla_unet_tensor_info(const bla_unet* m, int index, size_t* offset, size_t* count, char* name, int name_len) {
	BLA_REQUIRE(m && index >= 0 && index < (int)m->tensors.size(), BLA_ERR_INVALID, "tensor index out of range");
	const Tensor& t = m->tensors[index];
	if (offset) *offset = t.off;
	if (count) *count = t.count;
	if (name && name_len > 0) { strncpy(name, t.name.c_str(), name_len - 1); name[name_len - 1] = '\0'; }
	return BLA_OK;
}

/* forward(), model/cifar_unet.c:1099-1166; a batched model takes [B][C][H][W] images and [B][time_dim] embeddings */
bla_status bla_unet_forward_f32(bla_unet* m, void* stream, const float* d_x, const float* d_time_embedding, const unsigned char* d_drop) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(m && d_x && d_time_embedding, BLA_ERR_INVALID, "null argument");
	const bla_unet_config& c = m->cfg;
	const int* H = m->H; const int* W = m->W;
	const int B = m->batch;
	hipStream_t s = pick_stream(stream);
	m->last_x = d_x; m->last_temb = d_time_embedding;
	m->have_grads = false;
	if (m->time_jobs) {   // every block's time-embedding projection depends on the embedding alone: one launch for the 18 of them
		hipLaunchKernelGGL(time_dense_all_kernel, dim3(18, (unsigned)((B + 7) / 8), (unsigned)((m->max_cout + 63) / 64)), dim3(256),
		                   ((size_t)8 * c.time_dim + 4 * 8 * 64) * sizeof(float), s, m->time_jobs, d_time_embedding, B, c.time_dim);
		BLA_HIP(hipGetLastError());
	}
	if (m->n_prep_fwd) { st = conv_prepare_kernels(stream, m->prep_fwd, m->n_prep_fwd, m->prep_max); if (st) return st; }
	if (m->n_prep16_fwd) { st = bla_conv_bf16_prepare_kernels_table(stream, m->prep16_fwd, m->n_prep16_fwd, m->prep16_max_fwd); if (st) return st; }
	const unsigned char* drop = d_drop ? d_drop : m->zero_drop;   // the dropout decisions: block by block in forward order, inside a block image by image
	for (const Step& t : m->steps) {
		if (!step_runs(m, t)) continue;
		const float* in = t.in ? t.in : d_x;
		const int l = t.level;
		switch (t.kind) {
		case RES: st = m->stack->block_forward(m, stream, m->res[t.index], in, d_time_embedding, drop + m->res[t.index].drop_off * B); break;
		case ATT: st = att_forward(m, stream, m->att[t.index], in); break;
		case DOWN: case UP: case OUT_CONV: st = m->stack->conv_forward(m, stream, conv_of(m, t), in); break;
		case RESIZE: st = bla_nearest_neighbours_f32(stream, in, t.out, B * m->up[t.index].cin, H[l + 1], W[l + 1], H[l], W[l], 2); break;   // :1125-1131
		case CONCAT: st = concat(m, s, t); break;
		case OUT_NORM: st = bla_group_norm_relu_batched_f32(stream, B, in, t.out, m->out_sd, m->out_mu, c.dims[l], c.group_size, H[l] * W[l]); break;
		}
		if (st) return st;
	}
	return BLA_OK;
}

/* backward(), model/cifar_unet.c:1351-1436 (intended wiring, see the head of this file): fills the gradient bucket for the images, time
 * embeddings and dropout decisions of the last forward pass (summed over the images of a batch). */
/* the pass behind both entries: seeded with 2 (output - d_noise) by unet_loss_grad_kernel, or (d_noise NULL) with the caller's d_del_y, which is only read */
static bla_status unet_backward(bla_unet* m, void* stream, const float* d_noise, const float* d_del_y) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(m && (d_noise || d_del_y), BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(m->last_x, BLA_ERR_INVALID, "bla_unet_forward_f32 has not run");
	const bla_unet_config& c = m->cfg;
	const int* H = m->H; const int* W = m->W;
	const int B = m->batch;
	hipStream_t s = pick_stream(stream);
	if (m->n_prep_bwd) { st = conv_prepare_kernels(stream, m->prep_bwd, m->n_prep_bwd, m->prep_max); if (st) return st; }
	if (m->n_prep16_bwd) { st = bla_conv_bf16_prepare_kernels_table(stream, m->prep16_bwd, m->n_prep16_bwd, m->prep16_max_bwd); if (st) return st; }
	// Every gradient a step WRITES takes the next buffer: of three in rotation (a step reads the one written last and writes one, so never the one it reads),
	// or, with the weight gradients on the side lane, of the write-once pool -- what the lane still reads, the gradient a block or convolution came in with, is
	// never overwritten in this pass (create has counted the writes: backward_writes(m) <= kGradPool)
	size_t written = 0;
	auto next = [&]() -> float* { float* p = m->side ? m->gpool[written] : m->ring[written % 3]; written++; return p; };
	const int nout = (int)((size_t)c.in_channels * H[0] * W[0] * B);
	float* g = const_cast<float*>(d_del_y);   // the gradient that arrives at the step in hand (the caller's buffer: the last step only reads it, also from the side lane)
	if (d_noise) {
		g = next();
		hipLaunchKernelGGL(unet_loss_grad_kernel, dim3(grid_of((size_t)nout)), dim3(256), 0, s, m->outc.out, d_noise, g, nout);   // :1353-1364
		BLA_HIP(hipGetLastError());
	}
	for (size_t i = m->steps.size(); i-- > 0;) {
		const Step& t = m->steps[i];
		const int l = t.level;
		// a tapped output: the skip connection's gradient (left behind by its CONCAT's split) joins the main path's before the step sees it (:1405-1435)
		if (t.tap >= 0 && (st = bla_add_f32(stream, g, m->gskip[t.tap], level_floats(m, l) * B))) return st;
		if (!step_runs(m, t)) continue;
		const float* x = t.in ? t.in : m->last_x;   // the step's input in the forward pass
		float* out = i ? next() : nullptr;          // nothing consumes the gradient of the image: the first block forms its weight gradients only
		switch (t.kind) {
		case RES: st = m->stack->block_backward(m, stream, m->res[t.index], g, x, out); break;
		case ATT: st = att_backward(m, stream, m->att[t.index], g, x, out); break;
		case DOWN: case UP: case OUT_CONV: st = m->stack->conv_backward(m, stream, conv_of(m, t), g, x, out); break;
		case RESIZE: st = bla_nearest_neighbours_ddx_f32(stream, g, out, B * m->up[t.index].cin, H[l], W[l], H[l + 1], W[l + 1], 2); break;
		case CONCAT: st = split(m, s, t, g, out); break;
		case OUT_NORM:   // :1367-1369: the ReLU gate, then group norm
			st = bla_group_norm_ddx_gated_batched_f32(stream, B, g, out, x, m->out_mu, m->out_sd, c.dims[l], c.group_size, H[l] * W[l], t.out, nullptr);
			break;
		}
		if (st) return st;
		g = out;
	}
	if (m->defer_time_grads) {   // the 18 blocks' time-weight / time-bias gradients from the channel sums each block left behind (:1191-1199)
		hipLaunchKernelGGL(time_grads_all_kernel, dim3(18, (unsigned)((c.time_dim + 7) / 8)), dim3(256), 0, s, m->time_jobs, m->last_temb, B, c.time_dim);
		BLA_HIP(hipGetLastError());
	}
	if (m->side && (st = side_lane_join(s))) return st;      // the weight gradients are in when this stream moves on
	m->have_grads = true;
	return BLA_OK;
}

bla_status bla_unet_backward_f32(bla_unet* m, void* stream, const float* d_noise) {
	return unet_backward(m, stream, d_noise, nullptr);
}

bla_status bla_unet_backward_from_f32(bla_unet* m, void* stream, const float* d_del_y) {
	return unet_backward(m, stream, nullptr, d_del_y);
}

/* d_dtemb [B][time_dim] = dL/dtemb for the loss of the last backward pass: every block's time projection W_k [time_dim][cout] applied to the per-image
 * channel sums it left behind, summed over the 18 blocks -- one launch, nothing of the backward pass re-run or changed */
bla_status bla_unet_embedding_grad_f32(bla_unet* m, void* stream, float* d_dtemb) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(m && d_dtemb, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(m->have_grads, BLA_ERR_INVALID, "no bla_unet_backward_f32 since the last forward pass");
	const int tdim = m->cfg.time_dim;
	hipLaunchKernelGGL(temb_grad_all_kernel, dim3((unsigned)((tdim + 7) / 8), (unsigned)((m->batch + 7) / 8)), dim3(256), 0, pick_stream(stream), m->emb_jobs, m->batch,
	                   tdim, d_dtemb);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

}  // extern "C"
