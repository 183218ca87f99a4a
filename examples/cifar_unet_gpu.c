/* cifar_unet_gpu.c -- the reference's CIFAR-10 diffusion U-Net program (model/cifar_unet.c: `init`, `train <epochs>`, `run [<n>]`) as a C host
 * program over the batched device model of the C-ABI (include/bla.h, bla_unet_*).  Host code stays in C (gcc, C99); every pass runs on the GPU.
 *
 *   reference                                          here
 *   main()  :1940-1966  srand(42), three verbs         the same verbs and usage texts; the rand() stream of srand(42) kept in a state array of
 *                                                      this program's own (the GPU runtime draws from rand() too -- see mnist_nn_gpu.c)
 *   init()  :1846-1856  init_parameters + save         the same draws in the same order (:1804-1844) -- every ResNet block draws its 1x1
 *                                                      residual kernels whether forward() uses them or not (:1470), every up stage its
 *                                                      convolution (:1832,1836,1842) -- and the same file set below data/cifar_unet (:1545-1660)
 *   save_parameters :1545-1660                         byte for byte, the as-written quirks included: down_1/resnet_2 and up_N/resnet_1 are
 *                                                      written with fewer input channels than they have (3 instead of 128; the un-doubled
 *                                                      width), and the mid attention's five files land in mid/ beside an empty
 *                                                      mid/self_attention_0.  BLA_UNET_FULL_FILES=1 writes / reads every input channel instead.
 *   train() :1874-1934  ONE example: init_parameters,  `train <passes> [<batch>]`: init_parameters, then per pass `batch` examples, each drawn
 *     load_example, Gaussian noise, forward, MSE,      the way one call of the reference's train() draws its one: fill_random_data (rand()),
 *     backward; no update (the moment buffers are      3 x 32 x 32 values of random_gaussian on rand_r(&seed) with seed 0 carried on, the
 *     allocated and never used)                        dropout decisions of the 18 blocks in forward order (_dropout :1032-1042: one rand()
 *                                                      per element of the block's second ReLU).  One batched forward + backward on the GPU;
 *                                                      loss = mean over the batch of compute_mse_loss (:1858-1872); gradients are the sum over
 *                                                      the images.  `train 1` (batch 1) is exactly the reference's train().  The reference
 *                                                      has no update step; BLA_UNET_LEARN_RATE=x adds plain SGD (params -= x / batch * grads).
 *   run()   :1936-1938  empty                          `run [<n>]`: parameters from the files, n examples through forward(), mean loss printed
 *   time embedding: malloc'd, never written (:535)     zeros; BLA_UNET_TIMESTEP=t: relu(sinusoidal embedding of t) ("passed through ReLU
 *                                                      already", :168)
 *   fan_in = height x width of the resolution          the default.  With it the reference's own backward pass leaves fp32's range: group_norm
 *     (:1455,1474), whatever the channel count         divides by the VARIANCE (lib/norm.c:36-44), activations drift, and the gradient of the
 *                                                      reference's init reaches 1e72 in the reference's own fp64 arithmetic (measured with the
 *                                                      oracle, tests/test_c_unet.py).  BLA_UNET_INIT=unit draws the same rand() values onto
 *                                                      +-sqrt(3 / (values one output sums over)) instead: variance preserving, trainable.
 *   draws <images> <dir>                               host only (tests): everything `train 1 <images>` would hand the device, as raw files
 *   (not in the reference; what its train() / run()    `fit <epochs> [<batch>]` (default batch 64): DDPM training with Adam.  Parameters from
 *    were building towards: the Adam moments :1887,    draw_parameters() with the variance-preserving draw (BLA_UNET_INIT=reference: the
 *    the time embedding, an empty run() :1936)         reference's, which blows up, see above; BLA_UNET_RESUME=1: the file set).  Data: every
 *                                                      $BLA_CIFAR_DIR/data_batch_{1..5}.bin that exists (default data/cifar, at least one),
 *                                                      records in order, the last partial batch dropped, uploaded once as load_example maps
 *                                                      them.  Each pass: bla_diffusion_noise_f32 (t, eps, x_t, time embedding), dropout
 *                                                      decisions by bla_rand_bernoulli_u8 (p = DROPOUT_RATE), forward on x_t, backward
 *                                                      against eps, bla_adam_f32 with grad_scale 1 / batch.  The mean loss of the last
 *                                                      BLA_UNET_LOG_EVERY passes (default 50) is the only host round trip; the trained
 *                                                      parameters go to the file set at the end.  BLA_ADAM_LR (2e-4), BLA_DIFFUSION_STEPS
 *                                                      (1000, linear betas 1e-4 .. 0.02), BLA_SEED (42).  Draws nothing from rand() after
 *                                                      draw_parameters(): every random number is a Philox stream of BLA_SEED.
 *                                                      `sample <n> [<dir>]`: the file set, batches of min(n, BLA_UNET_BATCH) (default 16),
 *                                                      x_T = bla_rand_normal_f32(seed, offset 0), bla_unet_sample_f32, x_0 mapped back to
 *                                                      bytes (clamp(round((x + 1) 127.5)), the inverse of load_example) and written as
 *                                                      <dir>/sample_%04d.bmp (default data/cifar_unet_samples).  Batch k draws with seed
 *                                                      BLA_SEED + k.
 *   (not in the reference: its data_batch records'      Class-conditional diffusion with classifier-free guidance (Ho & Salimans 2022).
 *    label byte, read and dropped by load_example)     `fit` with BLA_UNET_CLASSES=1: the label bytes are read too (a label > 9 stops the
 *                                                      program before the device is opened); a [11][512] class table (row 10 = the null
 *                                                      class) starts at zero -- the conditional model starts exactly as the unconditional
 *                                                      one -- or, with BLA_UNET_RESUME=1, from class_embedding.csv if it exists.  Each pass:
 *                                                      noise, bla_class_embedding_f32 (label dropped with p = BLA_UNET_UNCOND, default 0.1,
 *                                                      Philox offset (pass << 32) + 2^31), dropout draw, forward, backward,
 *                                                      bla_unet_embedding_grad_f32, bla_class_embedding_grad_f32, Adam on the parameters and
 *                                                      on the table (moments of its own).  The table goes to <weights>/class_embedding.csv
 *                                                      (save_parameters' matrix format).  Without BLA_UNET_CLASSES `fit` is unchanged.
 *                                                      `sample` with BLA_UNET_CLASS=k (0..9): the table file (checked, like k, before the
 *                                                      device is opened) and bla_unet_sample_guided_f32 at model batch 2 x min(n,
 *                                                      BLA_UNET_BATCH), guidance BLA_UNET_GUIDANCE (default 3); file names, BMP format and
 *                                                      per-batch seeds as without.  Without BLA_UNET_CLASS `sample` is unchanged.
 *   (not in the reference)                             The weights DDPM samples from and few-step sampling (DDIM, Song, Meng, Ermon 2021).
 *                                                      `fit` with BLA_UNET_EMA=<decay> (0 < decay < 1, e.g. 0.9999): an exponential moving
 *                                                      average of the parameters (and of the class table when conditional) on the device,
 *                                                      started from the parameters fit starts from and updated by bla_ema_f32 after each
 *                                                      Adam step with min(decay, (1 + pass) / (10 + pass)); at the end a second, complete file
 *                                                      set below <weights>/ema/ (BLA_UNET_WEIGHTS=<weights>/ema samples from it).  With
 *                                                      BLA_UNET_RESUME=1 the average starts from <weights>/ema/ if that directory exists (a
 *                                                      missing file there stops the program before the device is opened), else from the
 *                                                      resumed parameters.  Without BLA_UNET_EMA `fit` writes what it wrote before.
 *                                                      `sample` with BLA_UNET_SAMPLE_STEPS=S (1 .. BLA_DIFFUSION_STEPS): the DDIM samplers
 *                                                      (guided with BLA_UNET_CLASS), S forward passes instead of BLA_DIFFUSION_STEPS;
 *                                                      BLA_UNET_ETA (0 .. 1, default 0: deterministic) scales the noise, BLA_UNET_CLIP=1
 *                                                      clamps the predicted x_0 to [-1, 1].  Bad values stop the program before the device is
 *                                                      opened.  Without BLA_UNET_SAMPLE_STEPS `sample` is unchanged.
 *   (not in the reference)                             DPM-Solver++(2M) (Lu et al. 2022), the second-order few-step sampler.  `sample` with
 *                                                      BLA_UNET_SAMPLER=dpmpp and BLA_UNET_SAMPLE_STEPS=S (required): bla_unet_sample_dpmpp_f32
 *                                                      (bla_unet_sample_guided_dpmpp_f32 with BLA_UNET_CLASS), S forward passes, deterministic;
 *                                                      BLA_UNET_SPACING=logsnr (default: timesteps uniform in log-SNR) or trailing (DDIM's);
 *                                                      BLA_UNET_CLIP as for DDIM.  BLA_UNET_SAMPLER=ddim names the DDIM samplers above.  Any
 *                                                      other sampler or spacing, a missing step count, or dpmpp with BLA_UNET_ETA other than 0
 *                                                      stops the program before the device is opened.  Without BLA_UNET_SAMPLER `sample` is
 *                                                      unchanged.
 *   (not in the reference)                             The rest of the DDPM training recipe (Ho et al. 2020), all on the device, all opt-in:
 *                                                      `fit` with BLA_UNET_SHUFFLE=1: every record is uploaded, epoch e takes the permutation
 *                                                      bla_rand_permutation_u32(records, BLA_SEED, (e << 32) + 2^31) and its pass k the entries
 *                                                      [k batch, (k + 1) batch), so the dropped tail differs per epoch (at most 2^20 records);
 *                                                      BLA_UNET_FLIP=1: each image mirrored left to right with probability 1/2.  Either one
 *                                                      makes the pass start with bla_diffusion_noise_gather_f32 (index, flips and labels in the
 *                                                      noising launch; without shuffling the index is 0, 1, 2, ...).  BLA_ADAM_CLIP_NORM=<x>
 *                                                      (x > 0, finite): the gradient of the whole model (the class table included) is clipped
 *                                                      to global norm x -- bla_memset, bla_sumsq_accumulate_f32 per bucket, bla_clip_scale_f32
 *                                                      with grad_scale 1 / batch, bla_adam_scaled_f32 -- and every logged pass prints a second
 *                                                      line, `Grad norm: <the last pass's norm before clipping>`.  BLA_ADAM_WARMUP=<n> (an
 *                                                      integer >= 1): pass p uses BLA_ADAM_LR * min(1, (p + 1) / n).  Bad values stop the
 *                                                      program before the device is opened.  With none of the four `fit` is unchanged.
 *
 *   (not in the reference)                             Held-out evaluation: the variational bound of Ho et al. 2020 (eq. 5) in bits/dim (bla.h).
 *                                                      `eval [<images>]`: BLA_CIFAR_EVAL_FILE (default $BLA_CIFAR_DIR/test_batch.bin) read as
 *                                                      fit reads its records, the first <images> (default all) in batches of BLA_UNET_BATCH
 *                                                      (default 64), the last partial batch dropped; the saved set, or the set below ema/ with
 *                                                      BLA_UNET_EVAL_EMA=1; BLA_UNET_CLASSES=1: every image with its own label's row (no label
 *                                                      dropout).  Timesteps: bla_diffusion_eval_timesteps of BLA_UNET_EVAL_STEPS (default
 *                                                      min(T - 1, 50)).  The batch that starts at record r is bla_unet_evaluate_f32 with
 *                                                      offset_base r x 3072 / 4 plus bla_diffusion_prior_kl_f32; the per-image doubles are copied
 *                                                      out once per batch and summed in record order.  Prints the image count, `Bits/dim:
 *                                                      <total> (prior, decoder, KL)` and the eps MSE per timestep.  A missing file, a bad option
 *                                                      or a bound that is not finite stops the program with status 1.
 *                                                      `fit` with BLA_UNET_EVAL_EVERY=<n> (an integer >= 1): the same evaluation of the live
 *                                                      weights every n passes and after the last, on the first BLA_UNET_EVAL_IMAGES records of
 *                                                      the evaluation file (default one batch; uploaded once), seed BLA_SEED, a fixed K; prints
 *                                                      `Held-out bits/dim: <total>` behind the pass's loss line.  Without it `fit` is unchanged.
 *
 *   (not in the reference)                             Training objectives beyond Ho et al. 2020, all opt-in.  `fit` with BLA_UNET_SCHEDULE=linear|cosine
 *                                                      (cosine: Nichol & Dhariwal 2021, bla_diffusion_cosine_betas(T, 0.008, 0.999)),
 *                                                      BLA_UNET_PREDICT=eps|x0|v (what the network predicts; v: Salimans & Ho 2022) and
 *                                                      BLA_UNET_MIN_SNR=<gamma> (Min-SNR-gamma loss weights, Hang et al. 2023; 0: none).  With any
 *                                                      of the three set the pass is noise, bla_diffusion_target_f32, forward,
 *                                                      bla_diffusion_loss_f32 (the gradient and the per-image losses), bla_unet_backward_from_f32
 *                                                      and the usual clip / Adam / EMA tail; the printed loss is the mean weighted loss; and fit
 *                                                      writes the line `schedule=... predict=... min_snr=...` to <weights>/objective.txt (and to
 *                                                      ema/objective.txt beside the averaged set).  `sample` and `eval` (and `fit` with
 *                                                      BLA_UNET_RESUME=1) read that file, build the diffusion object from it and call
 *                                                      bla_diffusion_set_objective; an option in the environment that contradicts the file, or a
 *                                                      malformed value, stops the program with status 1 before the device is opened.  A fit
 *                                                      without an objective removes an objective.txt that an earlier fit left beside a set it
 *                                                      overwrites.  With no option and no file every verb does exactly what it did before.
 *
 * BLA_UNET_DUMP=<dir> makes train write what it uploaded (params, x, time embedding, noise, dropout decisions) and what came back (prediction,
 * gradient bucket) as raw little-endian files; tests/test_c_unet.py compares those with the oracle.
 *
 * Paths: data/cifar_unet/... and data/cifar/data_batch_1.bin relative to the working directory, as in the reference (:49,1878);
 * BLA_UNET_WEIGHTS / BLA_CIFAR_BATCH override the directory / the file.
 *
 *   gcc -std=c99 -O2 -I include -I big-linear-algebra_amd/lib examples/cifar_unet_gpu.c -o cifar_unet_gpu \
 *       -L big-linear-algebra_amd/lib -l:libbla_host.so -L big-linear-algebra_amd/csrc -l:libbla_hip.so -lm */
#define _XOPEN_SOURCE 600      /* initstate / setstate, rand_r */
#include "bla.h"
#include "bmp.h"
#include "cifar10.h"
#include "csv.h"
#include "util.h"
#include <errno.h>
#include <fcntl.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

/* model/cifar_unet.c:26-37 */
enum { IMAGE_SIDE = 32, IMAGE_CHANNELS = 3, TIME_EMBED_DIM = 512, KERNEL_SIZE = 3, GROUP_SIZE = 32, KEY_DIM = 16, RESIZE_STRIDE = 2 };
static const int kDims[4] = {128, 256, 256, 256};
static const float DROPOUT_RATE = 0.1;
enum { IMAGE_FLOATS = IMAGE_CHANNELS * IMAGE_SIDE * IMAGE_SIDE, MAX_TENSORS = 160, MAX_BLOCKS = 18 };
enum { CLASSES = 10 };   /* CIFAR-10; the class table has CLASSES + 1 rows, the last the null class */

#define CHECK(call)                                                                              \
	do {                                                                                         \
		bla_status st_ = (call);                                                                 \
		if (st_ != BLA_OK) {                                                                     \
			fprintf(stderr, "%s failed: %s (%s)\n", #call, bla_status_string(st_), bla_last_error()); \
			exit(1);                                                                             \
		}                                                                                        \
	} while (0)

static char g_rng_mine[128];
static char* g_rng_others;
static void rng_begin(void) { g_rng_others = setstate(g_rng_mine); }
static void rng_end(void) { (void)setstate(g_rng_others); }
static void rng_seed(unsigned seed) { g_rng_others = initstate(seed, g_rng_mine, sizeof g_rng_mine); rng_end(); }

static const char* env_or(const char* name, const char* fallback) { const char* v = getenv(name); return v && *v ? v : fallback; }
static int env_flag(const char* name) { const char* v = getenv(name); return v && *v && strcmp(v, "0") != 0; }
static int side_of(int resolution) { int s = IMAGE_SIDE; for (int r = 1; r < resolution; r++) s = (s + RESIZE_STRIDE - 1) / RESIZE_STRIDE; return s; }   /* :39-46 */

/* BLA_UNET_HEADS=<n> (default 1): attention heads of width KEY_DIM in every self-attention block (bla_unet_create_heads); the attention
 * parameter files are then KEY_DIM x n wide.  Read before any sub-command opens the device: a value that is no positive integer, or one the model refuses
 * (no multi-head path for one of its blocks, or BLA_UNET_ATTENTION=bf16, which has no heads), stops every one of them. */
static int g_heads = 1;
static void heads_from_env(int attention) {
	const char* v = env_or("BLA_UNET_HEADS", "1");
	char* end;
	const long n = strtol(v, &end, 10);
	if (end == v || *end || n < 1 || n > 65536) { fprintf(stderr, "BLA_UNET_HEADS=%s: expected a positive integer\n", v); exit(1); }
	g_heads = (int)n;
	if (g_heads == 1) return;
	if (attention == BLA_UNET_ATTENTION_BF16) { fprintf(stderr, "BLA_UNET_HEADS=%s: BLA_UNET_ATTENTION=bf16 has no heads (f32 or online)\n", v); exit(1); }
	const int level[2] = {2, 4};   /* the resolutions with attention blocks */
	for (int i = 0; i < 2; i++) {
		const int c = kDims[level[i] - 1], s = side_of(level[i]) * side_of(level[i]);
		if (!bla_attention_f32_heads_applies(c, s, g_heads, KEY_DIM) && !bla_attention_online_bf16_heads_applies(c, s, g_heads, KEY_DIM) &&
		    !(attention == BLA_UNET_ATTENTION_F32_ONLINE && s > 64 && bla_attention_online_f32_applies(c, s, g_heads, KEY_DIM))) {
			fprintf(stderr, "BLA_UNET_HEADS=%s: the model refuses %d heads of width %d (C = %d, S = %d; heads x %d <= 256)\n", v, g_heads, KEY_DIM, c, s, KEY_DIM);
			exit(1);
		}
	}
}

/* ---- the parameter tensors, in init_parameters' order (:1804-1844) ------------------------------------------------------------------ */
typedef enum { DRAW_HE, DRAW_XAVIER, DRAW_ZERO } Draw;
typedef struct Tensor {
	char name[64];       /* the device model's name for it (the reference's struct members), "" = none */
	char file[96];       /* below the data directory */
	int rows, cols;      /* conv kernels: rows = out x in matrices of cols = k x k values ([out][in][k][k]); matrices: as allocated */
	int in, in_written;  /* conv kernels: input channels held / input channels save_parameters writes; 0 for a matrix */
	Draw draw;
	int fan_in, fan_out;
	int true_fan_in;     /* the values one output sums over: in x k x k of a kernel set, the rows of a matrix */
	float* host;         /* rows x cols */
} Tensor;
static Tensor g_tensors[MAX_TENSORS];
static int g_tensor_count;
static struct { int channels, side; } g_blocks[MAX_BLOCKS];   /* ResNet blocks in forward order: the shape of their dropout decisions */
static int g_block_count;
static char g_dirs[48][96];                                   /* directories save_parameters makes, in its order */
static int g_dir_count;

static Tensor* plan(const char* name, const char* file, int rows, int cols, int in, int in_written, Draw draw, int fan_in, int fan_out) {
	if (g_tensor_count == MAX_TENSORS) { fprintf(stderr, "tensor table full\n"); exit(1); }
	Tensor* t = &g_tensors[g_tensor_count++];
	snprintf(t->name, sizeof t->name, "%s", name);
	snprintf(t->file, sizeof t->file, "%s", file);
	t->rows = rows; t->cols = cols; t->in = in; t->in_written = in_written; t->draw = draw; t->fan_in = fan_in; t->fan_out = fan_out;
	t->true_fan_in = in ? in * cols : rows;
	t->host = calloc((size_t)rows * cols, sizeof(float));
	return t;
}
static void plan_dir(const char* dir) { snprintf(g_dirs[g_dir_count++], sizeof g_dirs[0], "%s", dir); }
static void plan_conv(const char* name, const char* file, int side, int in, int out, int k, int in_written) {
	plan(name, file, out * in, k * k, in, in_written, DRAW_HE, side * side, 0);          /* _init_conv_kernels :1454-1461: fan_in = height x width */
}
/* _init_resnet_block :1463-1471 / _save_resnet_block :1511-1526 */
static void plan_resnet(const char* member, const char* dir, int resolution, int in, int out, int in_written) {
	char name[64], file[96];
	const int side = side_of(resolution);
	plan_dir(dir);
	snprintf(name, sizeof name, "%s.conv_1_kernels", member); snprintf(file, sizeof file, "%s/conv_1.csv", dir);
	plan_conv(name, file, side, in, out, KERNEL_SIZE, in_written);
	snprintf(name, sizeof name, "%s.conv_2_kernels", member); snprintf(file, sizeof file, "%s/conv_2.csv", dir);
	plan_conv(name, file, side, out, out, KERNEL_SIZE, out);
	snprintf(name, sizeof name, "%s.time_weights", member); snprintf(file, sizeof file, "%s/time_weight.csv", dir);
	plan(name, file, TIME_EMBED_DIM, out, 0, 0, DRAW_HE, TIME_EMBED_DIM, 0);
	snprintf(name, sizeof name, "%s.time_biases", member); snprintf(file, sizeof file, "%s/time_bias.csv", dir);
	plan(name, file, 1, out, 0, 0, DRAW_ZERO, 0, 0);
	snprintf(name, sizeof name, "%s.residual_conv_kernels", member); snprintf(file, sizeof file, "%s/conv_3.csv", dir);
	plan_conv(in != out ? name : "", file, side, in, out, 1, in_written);                 /* drawn and saved always; used when in != out (:1062) */
	g_blocks[g_block_count].channels = out; g_blocks[g_block_count].side = side; g_block_count++;
}
/* _init_self_attention_block :1473-1482 / _save_self_attention_block :1528-1543; `dir` is made, the files go below `files_in` */
static void plan_attention(const char* member, const char* dir, const char* files_in, int resolution, int embed) {
	static const char* part[5] = {"Q_proj", "K_proj", "V_proj", "weights", "biases"}, *leaf[5] = {"query", "key", "value", "weight", "bias"};
	const int area = side_of(resolution) * side_of(resolution), width = KEY_DIM * g_heads;   /* the heads side by side */
	plan_dir(dir);
	for (int i = 0; i < 5; i++) {
		char name[64], file[96];
		snprintf(name, sizeof name, "%s.%s", member, part[i]); snprintf(file, sizeof file, "%s/%s.csv", files_in, leaf[i]);
		if (i < 2) plan(name, file, embed, width, 0, 0, DRAW_XAVIER, area, width);
		else if (i == 2) plan(name, file, embed, width, 0, 0, DRAW_HE, area, 0);
		else if (i == 3) plan(name, file, width, embed, 0, 0, DRAW_HE, width, 0);
		else plan(name, file, 1, embed, 0, 0, DRAW_ZERO, 0, 0);
	}
}
static void plan_model(void) {
	const int* D = kDims;
	const int full = env_flag("BLA_UNET_FULL_FILES");
	plan_dir("down_1");
	plan_resnet("down_1_resnet_1", "down_1/resnet_1", 1, IMAGE_CHANNELS, D[0], IMAGE_CHANNELS);
	plan_resnet("down_1_resnet_2", "down_1/resnet_2", 1, D[0], D[0], full ? D[0] : IMAGE_CHANNELS);        /* :1558 writes 3 input channels */
	plan_conv("down_1_conv_kernels", "down_1/conv_0.csv", side_of(1), D[0], D[1], KERNEL_SIZE, D[0]);
	plan_dir("down_2");
	plan_resnet("down_2_resnet_1", "down_2/resnet_1", 2, D[1], D[1], D[1]);
	plan_attention("down_2_self_attention_1", "down_2/self_attention_1", "down_2/self_attention_1", 2, D[1]);
	plan_resnet("down_2_resnet_2", "down_2/resnet_2", 2, D[1], D[1], D[1]);
	plan_attention("down_2_self_attention_2", "down_2/self_attention_2", "down_2/self_attention_2", 2, D[1]);
	plan_conv("down_2_conv_kernels", "down_2/conv_0.csv", side_of(2), D[1], D[2], KERNEL_SIZE, D[1]);
	plan_dir("down_3");
	plan_resnet("down_3_resnet_1", "down_3/resnet_1", 3, D[2], D[2], D[2]);
	plan_resnet("down_3_resnet_2", "down_3/resnet_2", 3, D[2], D[2], D[2]);
	plan_conv("down_3_conv_kernels", "down_3/conv_0.csv", side_of(3), D[2], D[3], KERNEL_SIZE, D[2]);
	plan_dir("down_4");
	plan_resnet("down_4_resnet_1", "down_4/resnet_1", 4, D[3], D[3], D[3]);
	plan_resnet("down_4_resnet_2", "down_4/resnet_2", 4, D[3], D[3], D[3]);
	plan_dir("mid");
	plan_resnet("mid_resnet_1", "mid/resnet_1", 4, D[3], D[3], D[3]);
	plan_attention("mid_self_attention", "mid/self_attention_0", full ? "mid/self_attention_0" : "mid", 4, D[3]);   /* :1612: position of mid/ */
	plan_resnet("mid_resnet_2", "mid/resnet_2", 4, D[3], D[3], D[3]);
	plan_dir("up_1");
	plan_resnet("up_1_resnet_1", "up_1/resnet_1", 4, 2 * D[3], D[3], full ? 2 * D[3] : D[3]);             /* :1621 and the other up_N/resnet_1: un-doubled */
	plan_resnet("up_1_resnet_2", "up_1/resnet_2", 4, D[3], D[3], D[3]);
	plan_conv(D[3] != D[2] ? "up_1_conv_kernels" : "", "up_1/conv_0.csv", side_of(3), D[3], D[2], KERNEL_SIZE, D[3]);
	plan_dir("up_2");
	plan_resnet("up_2_resnet_1", "up_2/resnet_1", 3, 2 * D[2], D[2], full ? 2 * D[2] : D[2]);
	plan_resnet("up_2_resnet_2", "up_2/resnet_2", 3, D[2], D[2], D[2]);
	plan_conv(D[2] != D[1] ? "up_2_conv_kernels" : "", "up_2/conv_0.csv", side_of(2), D[2], D[1], KERNEL_SIZE, D[2]);
	plan_dir("up_3");
	plan_resnet("up_3_resnet_1", "up_3/resnet_1", 2, 2 * D[1], D[1], full ? 2 * D[1] : D[1]);
	plan_attention("up_3_self_attention_1", "up_3/self_attention_1", "up_3/self_attention_1", 2, D[1]);
	plan_resnet("up_3_resnet_2", "up_3/resnet_2", 2, D[1], D[1], D[1]);
	plan_attention("up_3_self_attention_2", "up_3/self_attention_2", "up_3/self_attention_2", 2, D[1]);
	plan_conv(D[1] != D[0] ? "up_3_conv_kernels" : "", "up_3/conv_0.csv", side_of(1), D[1], D[0], KERNEL_SIZE, D[1]);
	plan_dir("up_4");
	plan_resnet("up_4_resnet_1", "up_4/resnet_1", 1, 2 * D[0], D[0], full ? 2 * D[0] : D[0]);
	plan_resnet("up_4_resnet_2", "up_4/resnet_2", 1, D[0], D[0], D[0]);
	plan_conv("output_conv_kernels", "output_conv.csv", side_of(1), D[0], IMAGE_CHANNELS, KERNEL_SIZE, D[0]);
}

/* init_parameters :1804-1844: _init_params_he / _init_params_xavier (:1439-1452) in double, stored as the float save_parameters would write */
static void draw_parameters(const char* default_init) {
	const int unit_gain = strcmp(env_or("BLA_UNET_INIT", default_init), "unit") == 0;
	rng_begin();
	for (int t = 0; t < g_tensor_count; t++) {
		Tensor* x = &g_tensors[t];
		const size_t n = (size_t)x->rows * x->cols;
		if (x->draw == DRAW_ZERO) { memset(x->host, 0, n * sizeof(float)); continue; }
		double scale = x->draw == DRAW_HE ? sqrt(6.0 / x->fan_in) : sqrt(6.0 / (x->fan_in + x->fan_out));
		if (unit_gain) scale = sqrt(3.0 / x->true_fan_in);
		for (size_t i = 0; i < n; i++) x->host[i] = (float)(2 * scale * (double)rand() / RAND_MAX - scale);
	}
	rng_end();
}

static const char* g_set = "";   /* "" = the parameter set, "ema" = fit's moving average of it, one directory below */
static void data_path(char* out, size_t n, const char* below) {
	snprintf(out, n, "%s%s%s%s%s", env_or("BLA_UNET_WEIGHTS", "data/cifar_unet"), *g_set ? "/" : "", g_set, *below ? "/" : "", below);
}

/* save_parameters :1545-1660 */
static void save_parameters(void) {
	char path[512];
	data_path(path, sizeof path, ""); mkdir(path, 0777);
	for (int d = 0; d < g_dir_count; d++) { data_path(path, sizeof path, g_dirs[d]); mkdir(path, 0777); }
	for (int t = 0; t < g_tensor_count; t++) {
		const Tensor* x = &g_tensors[t];
		data_path(path, sizeof path, x->file);
		if (!x->in || x->in_written == x->in) { write_csv_contents(path, x->host, x->cols, x->rows); continue; }
		/* _save_conv_kernels with fewer input channels than the kernels have (:1493-1509): the first in_written of every output channel */
		const int out = x->rows / x->in;
		float* part = malloc((size_t)out * x->in_written * x->cols * sizeof(float));
		for (int o = 0; o < out; o++) memcpy(part + (size_t)o * x->in_written * x->cols, x->host + (size_t)o * x->in * x->cols, (size_t)x->in_written * x->cols * sizeof(float));
		write_csv_contents(path, part, x->cols, out * x->in_written);
		free(part);
	}
}
/* load_parameters :1720-1802 (the same channel counts as save_parameters); input channels a file does not hold stay zero */
static void load_parameters(void) {
	char path[512];
	for (int t = 0; t < g_tensor_count; t++) {
		Tensor* x = &g_tensors[t];
		data_path(path, sizeof path, x->file);
		FILE* f = fopen(path, "r");
		if (!f) { fprintf(stderr, "cannot open %s (run `init` first)\n", path); exit(1); }
		int count = 0;
		float* v = read_csv_contents_file(f, &count);
		const int in_file = x->in ? x->in_written : 0, out = x->in ? x->rows / x->in : 0;
		const size_t want = x->in ? (size_t)out * in_file * x->cols : (size_t)x->rows * x->cols;
		if ((size_t)count != want) { fprintf(stderr, "%s holds %d values, expected %zu\n", path, count, want); exit(1); }
		memset(x->host, 0, (size_t)x->rows * x->cols * sizeof(float));
		if (!x->in) memcpy(x->host, v, want * sizeof(float));
		else for (int o = 0; o < out; o++) memcpy(x->host + (size_t)o * x->in * x->cols, v + (size_t)o * in_file * x->cols, (size_t)in_file * x->cols * sizeof(float));
		free(v);
	}
}

/* ---- one example the way train() makes it (:1903-1914) + the dropout decisions forward() would draw (:1032-1042) ---------------------- */
typedef struct Inputs {
	int batch;
	size_t drop_per_image;       /* sum over the blocks */
	float *x, *noise, *temb;     /* [B][3][32][32], [B][3][32][32], [B][512] */
	unsigned char* drop;         /* device layout: block by block, inside a block image by image */
} Inputs;
static Inputs inputs_alloc(int batch) {
	Inputs in; in.batch = batch; in.drop_per_image = 0;
	for (int b = 0; b < g_block_count; b++) in.drop_per_image += (size_t)g_blocks[b].channels * g_blocks[b].side * g_blocks[b].side;
	in.x = malloc((size_t)batch * IMAGE_FLOATS * sizeof(float)); in.noise = malloc((size_t)batch * IMAGE_FLOATS * sizeof(float));
	in.temb = calloc((size_t)batch * TIME_EMBED_DIM, sizeof(float)); in.drop = malloc(in.drop_per_image * batch);
	return in;
}
static void inputs_free(Inputs* in) { free(in->x); free(in->noise); free(in->temb); free(in->drop); }
static void time_embedding(float* out) {
	const char* v = getenv("BLA_UNET_TIMESTEP");
	memset(out, 0, TIME_EMBED_DIM * sizeof(float));
	if (!v || !*v) return;
	const double t = atof(v); const int half = TIME_EMBED_DIM / 2;
	for (int i = 0; i < half; i++) {
		const double w = exp(-log(10000.0) * i / half), s = sin(t * w), c = cos(t * w);
		out[i] = (float)(s > 0 ? s : 0); out[half + i] = (float)(c > 0 ? c : 0);
	}
}
static void draw_inputs(Inputs* in, int fd, unsigned int* noise_seed, int with_dropout) {
	uint8_t pixels[3072];
	rng_begin();
	for (int b = 0; b < in->batch; b++) {
		fill_random_data(fd, pixels);                                                           /* load_example :221-233 */
		for (int i = 0; i < IMAGE_FLOATS; i++) in->x[(size_t)b * IMAGE_FLOATS + i] = (float)(((double)pixels[i] - 127.5) / 127.5);
		for (int i = 0; i < IMAGE_FLOATS; i++) in->noise[(size_t)b * IMAGE_FLOATS + i] = (float)random_gaussian(noise_seed);
		time_embedding(in->temb + (size_t)b * TIME_EMBED_DIM);
		size_t at = 0;
		for (int k = 0; k < g_block_count; k++) {
			const size_t n = (size_t)g_blocks[k].channels * g_blocks[k].side * g_blocks[k].side;
			unsigned char* d = in->drop + at * in->batch + (size_t)b * n;
			for (size_t i = 0; i < n; i++) d[i] = with_dropout ? (float)rand() / RAND_MAX < DROPOUT_RATE : 0;
			at += n;
		}
	}
	rng_end();
}
static int open_batch_file(void) {
	const char* path = env_or("BLA_CIFAR_BATCH", "data/cifar/data_batch_1.bin");                /* :1878 */
	const int fd = open(path, O_RDONLY);
	if (fd < 0) { fprintf(stderr, "cannot open %s: %s\n", path, strerror(errno)); exit(1); }
	return fd;
}
static void dump(const char* dir, const char* leaf, const void* data, size_t bytes) {
	char path[512];
	snprintf(path, sizeof path, "%s/%s", dir, leaf);
	FILE* f = fopen(path, "wb");
	if (!f || fwrite(data, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path); exit(1); }
	fclose(f);
}

/* ---- the device model ----------------------------------------------------------------------------------------------------------------- */
typedef struct Device {
	bla_unet* net;
	int batch;
	float *x, *noise, *temb;
	unsigned char* drop;
	float* bucket;     /* host image of the parameter bucket */
} Device;
/* BLA_UNET_PRODUCTS=f32|bf16 (default f32): the precision of the model's convolution products (bla_unet_create_mixed).  The parameter files are fp32 in
 * both modes: weights trained in one load in the other. */
static int g_products = BLA_UNET_PRODUCTS_F32;
static void products_from_env(void) {
	const char* v = env_or("BLA_UNET_PRODUCTS", "f32");
	if (strcmp(v, "f32") == 0) g_products = BLA_UNET_PRODUCTS_F32;
	else if (strcmp(v, "bf16") == 0) g_products = BLA_UNET_PRODUCTS_BF16;
	else { fprintf(stderr, "BLA_UNET_PRODUCTS=%s: expected f32 or bf16\n", v); exit(1); }
}
/* BLA_UNET_ATTENTION=f32|bf16|online|online-f32 (default f32): where the model's attention blocks multiply (bla_unet_set_attention; online =
 * bf16 products with the online softmax, any block up to S = 4096; online-f32 = the online softmax in fp32 for every block with S > 64, the model created in
 * that mode by bla_unet_create_attention); orthogonal to the above. */
static int g_attention = BLA_UNET_ATTENTION_F32;
static void attention_from_env(void) {
	const char* v = env_or("BLA_UNET_ATTENTION", "f32");
	if (strcmp(v, "f32") == 0) g_attention = BLA_UNET_ATTENTION_F32;
	else if (strcmp(v, "bf16") == 0) g_attention = BLA_UNET_ATTENTION_BF16;
	else if (strcmp(v, "online") == 0) g_attention = BLA_UNET_ATTENTION_BF16_ONLINE;
	else if (strcmp(v, "online-f32") == 0) g_attention = BLA_UNET_ATTENTION_F32_ONLINE;
	else { fprintf(stderr, "BLA_UNET_ATTENTION=%s: expected f32, bf16, online or online-f32\n", v); exit(1); }
}
static Device device_open(int batch, size_t drop_per_image) {
	Device dv; memset(&dv, 0, sizeof dv); dv.batch = batch;
	CHECK(bla_init(atoi(env_or("BLA_DEVICE", "0"))));
	bla_unet_config cfg = {IMAGE_SIDE, IMAGE_SIDE, IMAGE_CHANNELS, {kDims[0], kDims[1], kDims[2], kDims[3]}, TIME_EMBED_DIM, KERNEL_SIZE, GROUP_SIZE, KEY_DIM};
	if (g_attention == BLA_UNET_ATTENTION_F32_ONLINE) CHECK(bla_unet_create_attention(&dv.net, &cfg, batch, g_products, g_heads, g_attention));
	else {
		CHECK(bla_unet_create_heads(&dv.net, &cfg, batch, g_products, g_heads));
		CHECK(bla_unet_set_attention(dv.net, g_attention));
	}
	if (bla_unet_dropout_count(dv.net) != drop_per_image * batch) { fprintf(stderr, "dropout layout: device %zu, host %zu\n", bla_unet_dropout_count(dv.net), drop_per_image * batch); exit(1); }
	CHECK(bla_malloc((void**)&dv.x, (size_t)batch * IMAGE_FLOATS * sizeof(float)));
	CHECK(bla_malloc((void**)&dv.noise, (size_t)batch * IMAGE_FLOATS * sizeof(float)));
	CHECK(bla_malloc((void**)&dv.temb, (size_t)batch * TIME_EMBED_DIM * sizeof(float)));
	CHECK(bla_malloc((void**)&dv.drop, drop_per_image * batch));
	dv.bucket = calloc(bla_unet_param_count(dv.net), sizeof(float));
	return dv;
}
/* host tensors -> bucket -> device; every device tensor must be fed by exactly one host tensor */
static void device_set_params(Device* dv) {
	const int n = bla_unet_tensor_count(dv->net);
	int fed = 0;
	for (int i = 0; i < n; i++) {
		size_t off, count; char name[64];
		CHECK(bla_unet_tensor_info(dv->net, i, &off, &count, name, sizeof name));
		for (int t = 0; t < g_tensor_count; t++) {
			const Tensor* x = &g_tensors[t];
			if (strcmp(x->name, name) != 0) continue;
			if ((size_t)x->rows * x->cols != count) { fprintf(stderr, "%s: device %zu values, host %d\n", name, count, x->rows * x->cols); exit(1); }
			memcpy(dv->bucket + off, x->host, count * sizeof(float)); fed++;
		}
	}
	if (fed != n) { fprintf(stderr, "%d of the device model's %d tensors have a host tensor\n", fed, n); exit(1); }
	CHECK(bla_memcpy_h2d(bla_unet_params(dv->net), dv->bucket, bla_unet_param_count(dv->net) * sizeof(float), NULL));
}
static void device_upload(Device* dv, const Inputs* in) {
	CHECK(bla_memcpy_h2d(dv->x, in->x, (size_t)in->batch * IMAGE_FLOATS * sizeof(float), NULL));
	CHECK(bla_memcpy_h2d(dv->noise, in->noise, (size_t)in->batch * IMAGE_FLOATS * sizeof(float), NULL));
	CHECK(bla_memcpy_h2d(dv->temb, in->temb, (size_t)in->batch * TIME_EMBED_DIM * sizeof(float), NULL));
	CHECK(bla_memcpy_h2d(dv->drop, in->drop, in->drop_per_image * in->batch, NULL));
}
/* device bucket -> host tensors (the inverse of device_set_params) */
static void device_get_params(Device* dv) {
	CHECK(bla_memcpy_d2h(dv->bucket, bla_unet_params(dv->net), bla_unet_param_count(dv->net) * sizeof(float), NULL));
	CHECK(bla_stream_sync(NULL));
	const int n = bla_unet_tensor_count(dv->net);
	for (int i = 0; i < n; i++) {
		size_t off, count; char name[64];
		CHECK(bla_unet_tensor_info(dv->net, i, &off, &count, name, sizeof name));
		for (int t = 0; t < g_tensor_count; t++) if (strcmp(g_tensors[t].name, name) == 0) memcpy(g_tensors[t].host, dv->bucket + off, count * sizeof(float));
	}
}
static void device_close(Device* dv) {
	CHECK(bla_free(dv->x)); CHECK(bla_free(dv->noise)); CHECK(bla_free(dv->temb)); CHECK(bla_free(dv->drop));
	CHECK(bla_unet_destroy(dv->net)); free(dv->bucket);
	CHECK(bla_shutdown());
}
/* compute_mse_loss :1858-1872 per image (float accumulation in the reference's order), averaged over the batch */
static float batch_loss(const float* prediction, const float* noise, int batch) {
	double total = 0;
	for (int b = 0; b < batch; b++) {
		float loss = 0;
		for (int i = 0; i < IMAGE_FLOATS; i++) { const float r = prediction[(size_t)b * IMAGE_FLOATS + i] - noise[(size_t)b * IMAGE_FLOATS + i]; loss += r * r; }
		total += loss / IMAGE_FLOATS;
	}
	return (float)(total / batch);
}

static void init(void) {
	draw_parameters("reference");
	save_parameters();
}

static void train(int passes, int batch) {
	const int fd = open_batch_file();
	const char* dump_dir = getenv("BLA_UNET_DUMP");
	const double learn_rate = atof(env_or("BLA_UNET_LEARN_RATE", "0"));
	draw_parameters("reference");                                                               /* :1900 (load_parameters is commented out there) */
	Inputs in = inputs_alloc(batch);
	Device dv = device_open(batch, in.drop_per_image);
	device_set_params(&dv);
	const size_t params = bla_unet_param_count(dv.net);
	float* prediction = malloc((size_t)batch * IMAGE_FLOATS * sizeof(float));
	unsigned int seed = 0;                                                                      /* :1902 */
	for (int pass = 0; pass < passes; pass++) {
		draw_inputs(&in, fd, &seed, 1);
		device_upload(&dv, &in);
		CHECK(bla_unet_forward_f32(dv.net, NULL, dv.x, dv.temb, dv.drop));
		CHECK(bla_unet_backward_f32(dv.net, NULL, dv.noise));
		CHECK(bla_memcpy_d2h(prediction, bla_unet_output(dv.net), (size_t)batch * IMAGE_FLOATS * sizeof(float), NULL));
		CHECK(bla_stream_sync(NULL));
		printf("Pass %d:\tAvg loss: %f\n", pass, batch_loss(prediction, in.noise, batch));
		if (dump_dir && pass == passes - 1) {
			float* grads = malloc(params * sizeof(float));
			CHECK(bla_memcpy_d2h(grads, bla_unet_grads(dv.net), params * sizeof(float), NULL));
			CHECK(bla_stream_sync(NULL));
			CHECK(bla_memcpy_d2h(dv.bucket, bla_unet_params(dv.net), params * sizeof(float), NULL));
			CHECK(bla_stream_sync(NULL));
			dump(dump_dir, "params.f32", dv.bucket, params * sizeof(float)); dump(dump_dir, "grads.f32", grads, params * sizeof(float));
			dump(dump_dir, "x.f32", in.x, (size_t)batch * IMAGE_FLOATS * sizeof(float)); dump(dump_dir, "noise.f32", in.noise, (size_t)batch * IMAGE_FLOATS * sizeof(float));
			dump(dump_dir, "temb.f32", in.temb, (size_t)batch * TIME_EMBED_DIM * sizeof(float)); dump(dump_dir, "drop.u8", in.drop, in.drop_per_image * batch);
			dump(dump_dir, "prediction.f32", prediction, (size_t)batch * IMAGE_FLOATS * sizeof(float));
			free(grads);
		}
		if (learn_rate != 0) {                                                                  /* not in the reference: plain SGD on the batch mean */
			CHECK(bla_scale_f32(NULL, bla_unet_grads(dv.net), params, (float)(-learn_rate / batch)));
			CHECK(bla_add_f32(NULL, bla_unet_params(dv.net), bla_unet_grads(dv.net), params));
		}
	}
	if (learn_rate != 0) {                                                                      /* trained parameters back into the file set */
		device_get_params(&dv);
		save_parameters();
	}
	free(prediction); inputs_free(&in); device_close(&dv); close(fd);
}

static void run(int num_predictions) {
	const int fd = open_batch_file();
	int batch = atoi(env_or("BLA_UNET_BATCH", "16"));
	if (batch > num_predictions) batch = num_predictions;
	if (batch < 1) { close(fd); return; }
	load_parameters();
	Inputs in = inputs_alloc(batch);
	Device dv = device_open(batch, in.drop_per_image);
	device_set_params(&dv);
	float* prediction = malloc((size_t)batch * IMAGE_FLOATS * sizeof(float));
	unsigned int seed = 0;
	double total = 0; int done = 0;
	printf("Predicting the noise of %d examples...", num_predictions);
	while (done < num_predictions) {
		draw_inputs(&in, fd, &seed, 0);                                                         /* inference: nothing dropped */
		device_upload(&dv, &in);
		CHECK(bla_unet_forward_f32(dv.net, NULL, dv.x, dv.temb, NULL));
		CHECK(bla_memcpy_d2h(prediction, bla_unet_output(dv.net), (size_t)batch * IMAGE_FLOATS * sizeof(float), NULL));
		CHECK(bla_stream_sync(NULL));
		const int take = num_predictions - done < batch ? num_predictions - done : batch;       /* a last, partial batch counts its first images */
		total += (double)batch_loss(prediction, in.noise, take) * take; done += take;
	}
	printf("done! Avg loss: %f\n", total / num_predictions);
	free(prediction); inputs_free(&in); device_close(&dv); close(fd);
}

/* host only: what `train 1 <images>` would upload, and the rand() value that would come next */
static void draws(int images, const char* dir) {
	const int fd = open_batch_file();
	draw_parameters("reference");
	Inputs in = inputs_alloc(images);
	unsigned int seed = 0;
	draw_inputs(&in, fd, &seed, 1);
	dump(dir, "x.f32", in.x, (size_t)images * IMAGE_FLOATS * sizeof(float)); dump(dir, "noise.f32", in.noise, (size_t)images * IMAGE_FLOATS * sizeof(float));
	dump(dir, "drop.u8", in.drop, in.drop_per_image * images);
	char path[512];
	snprintf(path, sizeof path, "%s/params.f32", dir);                                          /* the tensors the device model has, in init order */
	FILE* f = fopen(path, "wb");
	for (int t = 0; f && t < g_tensor_count; t++)
		if (g_tensors[t].name[0]) fwrite(g_tensors[t].host, sizeof(float), (size_t)g_tensors[t].rows * g_tensors[t].cols, f);
	if (!f || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", path); exit(1); }
	rng_begin(); const int next = rand(); rng_end();
	printf("blocks %d drop_per_image %zu next_rand %d\n", g_block_count, in.drop_per_image, next);
	inputs_free(&in); close(fd);
}

/* ---- fit / sample: DDPM training with Adam and the reverse-diffusion sampler (not in the reference; see the head of this file) ------------ */
static unsigned long long env_seed(void) { return strtoull(env_or("BLA_SEED", "42"), NULL, 10); }
static int env_steps(void) { const int T = atoi(env_or("BLA_DIFFUSION_STEPS", "1000")); if (T < 1) { fprintf(stderr, "BLA_DIFFUSION_STEPS must be >= 1\n"); exit(1); } return T; }

/* the records of one CIFAR-10 binary file appended to *all (and their label bytes to *lab, if not NULL), mapped as load_example maps them (:221-233:
 * planes with their rows flipped, (p - 127.5) / 127.5); *n counts the records held */
static void read_records(FILE* f, float** all, size_t* n, uint8_t** lab) {
	uint8_t rec[3073];
	while (fread(rec, 1, sizeof rec, f) == sizeof rec) {
		if (*n % 1024 == 0) { *all = realloc(*all, (*n + 1024) * IMAGE_FLOATS * sizeof(float)); if (lab) *lab = realloc(*lab, *n + 1024); }
		if (lab) (*lab)[*n] = rec[0];
		float* x = *all + *n * IMAGE_FLOATS;
		for (int c = 0; c < IMAGE_CHANNELS; c++)
			for (int y = 0; y < IMAGE_SIDE; y++)
				for (int i = 0; i < IMAGE_SIDE; i++)
					x[(c * IMAGE_SIDE + y) * IMAGE_SIDE + i] = (float)(((double)rec[1 + (c * IMAGE_SIDE + IMAGE_SIDE - 1 - y) * IMAGE_SIDE + i] - 127.5) / 127.5);
		(*n)++;
	}
}

/* every data_batch_{1..5}.bin below BLA_CIFAR_DIR, records in order, mapped as load_example maps them (:221-233: planes with their rows flipped,
 * (p - 127.5) / 127.5); *count = records read; *labels (if not NULL): the records' label bytes */
static float* read_training_set(size_t* count, uint8_t** labels) {
	const char* dir = env_or("BLA_CIFAR_DIR", "data/cifar");
	float* all = NULL; size_t n = 0;
	uint8_t* lab = NULL;
	int files = 0;
	for (int k = 1; k <= 5; k++) {
		char path[512];
		snprintf(path, sizeof path, "%s/data_batch_%d.bin", dir, k);
		FILE* f = fopen(path, "rb");
		if (!f) {
			if (k == 1 && errno != ENOENT) { fprintf(stderr, "cannot open %s: %s\n", path, strerror(errno)); exit(1); }
			continue;
		}
		files++;
		read_records(f, &all, &n, labels ? &lab : NULL);
		fclose(f);
	}
	if (!files) { fprintf(stderr, "cannot open %s/data_batch_1.bin: %s (nor any data_batch_{2..5}.bin)\n", dir, strerror(ENOENT)); exit(1); }
	*count = n;
	if (labels) *labels = lab;
	return all;
}

/* the class table, <weights>/class_embedding.csv, [CLASSES + 1][TIME_EMBED_DIM] in save_parameters' matrix format; 0 = no such file */
static int load_class_table(float* table) {
	char path[512];
	data_path(path, sizeof path, "class_embedding.csv");
	FILE* f = fopen(path, "r");
	if (!f) return 0;
	int count = 0;
	float* v = read_csv_contents_file(f, &count);
	if (count != (CLASSES + 1) * TIME_EMBED_DIM) { fprintf(stderr, "%s holds %d values, expected %d\n", path, count, (CLASSES + 1) * TIME_EMBED_DIM); exit(1); }
	memcpy(table, v, (size_t)count * sizeof(float));
	free(v);
	return 1;
}
static void save_class_table(float* table) {
	char path[512];
	data_path(path, sizeof path, "class_embedding.csv");
	write_csv_contents(path, table, TIME_EMBED_DIM, CLASSES + 1);
}

/* BLA_UNET_EMA=<decay> for fit, 0 < decay < 1; 0 = not set */
static double env_ema_decay(void) {
	const char* v = getenv("BLA_UNET_EMA");
	if (!v || !*v) return 0;
	char* end = NULL;
	const double decay = strtod(v, &end);
	if (*end || !(decay > 0 && decay < 1)) { fprintf(stderr, "fit: BLA_UNET_EMA=%s; the decay must lie strictly between 0 and 1 (e.g. 0.9999)\n", v); exit(1); }
	return decay;
}
/* a flag of fit that takes 0 or 1 and nothing else (unset or empty: 0) */
static int env_fit_flag(const char* name) {
	const char* v = getenv(name);
	if (!v || !*v || strcmp(v, "0") == 0) return 0;
	if (strcmp(v, "1") != 0) { fprintf(stderr, "fit: %s=%s; the value must be 0 or 1\n", name, v); exit(1); }
	return 1;
}
/* BLA_ADAM_CLIP_NORM=<x> for fit, x > 0 and finite; 0 = not set */
static double env_clip_norm(void) {
	const char* v = getenv("BLA_ADAM_CLIP_NORM");
	if (!v || !*v) return 0;
	char* end = NULL;
	const double x = strtod(v, &end);
	if (*end || !(x > 0) || !isfinite(x) || !isfinite((float)x)) { fprintf(stderr, "fit: BLA_ADAM_CLIP_NORM=%s; the norm must be positive and finite (e.g. 1)\n", v); exit(1); }
	return x;
}
/* BLA_ADAM_WARMUP=<n> for fit, an integer >= 1; 0 = not set */
static long env_warmup(void) {
	const char* v = getenv("BLA_ADAM_WARMUP");
	if (!v || !*v) return 0;
	char* end = NULL;
	errno = 0;
	const long n = strtol(v, &end, 10);
	if (*end || errno || n < 1) { fprintf(stderr, "fit: BLA_ADAM_WARMUP=%s; the warm-up is a whole number of passes >= 1\n", v); exit(1); }
	return n;
}
/* BLA_UNET_EVAL_EVERY=<n> for fit, an integer >= 1; 0 = not set */
static long env_eval_every(void) {
	const char* v = getenv("BLA_UNET_EVAL_EVERY");
	if (!v || !*v) return 0;
	char* end = NULL;
	errno = 0;
	const long n = strtol(v, &end, 10);
	if (*end || errno || n < 1) { fprintf(stderr, "fit: BLA_UNET_EVAL_EVERY=%s; the evaluation runs every whole number of passes >= 1\n", v); exit(1); }
	return n;
}
/* ---- the training objective: BLA_UNET_SCHEDULE, BLA_UNET_PREDICT, BLA_UNET_MIN_SNR and <weights>/objective.txt (see the head of this file) --------- */
typedef struct Objective {
	int active;              /* an option is set or the file exists: fit takes the objective pass and writes the file */
	int cosine, predict;     /* predict: BLA_PREDICT_* */
	double gamma;
	char gamma_text[32];     /* gamma as it was given, for the file */
} Objective;
static int parse_schedule(const char* verb, const char* from, const char* v) {
	if (strcmp(v, "linear") == 0) return 0;
	if (strcmp(v, "cosine") == 0) return 1;
	fprintf(stderr, "%s: %sBLA_UNET_SCHEDULE=%s; the schedules are linear and cosine\n", verb, from, v);
	exit(1);
}
static int parse_predict(const char* verb, const char* from, const char* v) {
	if (strcmp(v, "eps") == 0) return BLA_PREDICT_EPS;
	if (strcmp(v, "x0") == 0) return BLA_PREDICT_X0;
	if (strcmp(v, "v") == 0) return BLA_PREDICT_V;
	fprintf(stderr, "%s: %sBLA_UNET_PREDICT=%s; the network predicts eps, x0 or v\n", verb, from, v);
	exit(1);
}
static double parse_min_snr(const char* verb, const char* from, const char* v) {
	char* end = NULL;
	const double g = strtod(v, &end);
	if (end == v || *end || !(g >= 0) || !isfinite(g) || strlen(v) >= sizeof ((Objective*)0)->gamma_text || v[0] == ' ' || v[0] == '\t' || v[0] == '\n') {
		fprintf(stderr, "%s: %sBLA_UNET_MIN_SNR=%s; gamma is a finite number >= 0 (0: no weighting; e.g. 5)\n", verb, from, v);
		exit(1);
	}
	return g;
}
static const char* schedule_name(int cosine) { return cosine ? "cosine" : "linear"; }
static const char* predict_name(int predict) { return predict == BLA_PREDICT_V ? "v" : (predict == BLA_PREDICT_X0 ? "x0" : "eps"); }
/* The options of the environment, checked; with use_file the line fit wrote to <weights>/objective.txt fills in what the environment leaves open, and an
 * option that contradicts it stops the program.  Nothing here needs the device. */
static Objective resolve_objective(const char* verb, int use_file) {
	Objective o; memset(&o, 0, sizeof o);
	strcpy(o.gamma_text, "0");
	const char *se = getenv("BLA_UNET_SCHEDULE"), *pe = getenv("BLA_UNET_PREDICT"), *ge = getenv("BLA_UNET_MIN_SNR");
	if (se && !*se) se = NULL;
	if (pe && !*pe) pe = NULL;
	if (ge && !*ge) ge = NULL;
	if (se) o.cosine = parse_schedule(verb, "", se);
	if (pe) o.predict = parse_predict(verb, "", pe);
	if (ge) { o.gamma = parse_min_snr(verb, "", ge); strcpy(o.gamma_text, ge); }
	o.active = se || pe || ge;
	char path[512];
	data_path(path, sizeof path, "objective.txt");
	FILE* f = use_file ? fopen(path, "r") : NULL;
	if (!f) return o;
	char sv[16], pv[16], gv[64], from[600];
	const int got = fscanf(f, "schedule=%15s predict=%15s min_snr=%63s", sv, pv, gv);
	fclose(f);
	if (got != 3) { fprintf(stderr, "%s: %s does not hold the line `schedule=... predict=... min_snr=...` that fit writes\n", verb, path); exit(1); }
	snprintf(from, sizeof from, "%s: ", path);
	const int cosine = parse_schedule(verb, from, sv), predict = parse_predict(verb, from, pv);
	const double gamma = parse_min_snr(verb, from, gv);
	if ((se && cosine != o.cosine) || (pe && predict != o.predict) || (ge && gamma != o.gamma)) {
		fprintf(stderr, "%s: the environment asks for schedule=%s predict=%s min_snr=%s, but the weights were trained with `schedule=%s predict=%s min_snr=%s` (%s)\n",
		        verb, se ? se : "(unset)", pe ? pe : "(unset)", ge ? ge : "(unset)", sv, pv, gv, path);
		exit(1);
	}
	o.cosine = cosine; o.predict = predict; o.gamma = gamma; strcpy(o.gamma_text, gv);
	o.active = 1;
	return o;
}
/* beside the parameter set just saved (data_path: the set below ema/ gets its own copy) */
static void save_objective(const Objective* o) {
	char path[512];
	data_path(path, sizeof path, "objective.txt");
	FILE* f = fopen(path, "w");
	if (!f || fprintf(f, "schedule=%s predict=%s min_snr=%s\n", schedule_name(o->cosine), predict_name(o->predict), o->gamma_text) < 0 || fclose(f) != 0) {
		fprintf(stderr, "cannot write %s\n", path);
		exit(1);
	}
}
/* a set saved by a fit without an objective is an eps model on the linear schedule: a file left beside it by an earlier fit into the same directory
 * would make sample and eval read it as something else */
static void remove_objective(void) {
	char path[512];
	data_path(path, sizeof path, "objective.txt");
	if (remove(path) != 0 && errno != ENOENT) { fprintf(stderr, "cannot remove %s: %s\n", path, strerror(errno)); exit(1); }
}
/* the diffusion object of an objective: the linear betas 1e-4 .. 0.02 as ever, or the cosine betas (s = 0.008, capped at 0.999); set_objective only where
 * an objective is in force, so that without one the object is the one this program has always made */
static bla_diffusion* open_diffusion(const Objective* o, int T) {
	bla_diffusion* diff;
	if (o->cosine) {
		double* betas = malloc((size_t)T * sizeof(double));
		CHECK(bla_diffusion_cosine_betas(T, 0.008, 0.999, betas));
		CHECK(bla_diffusion_create_from_betas(&diff, T, betas));
		free(betas);
	} else {
		CHECK(bla_diffusion_create(&diff, T, 1e-4f, 0.02f));
	}
	if (o->active) CHECK(bla_diffusion_set_objective(diff, o->predict, o->gamma));
	return diff;
}

/* exchanges the host tensors with another set of the same shapes */
static void swap_sets(float** other) {
	for (int t = 0; t < g_tensor_count; t++) { float* h = g_tensors[t].host; g_tensors[t].host = other[t]; other[t] = h; }
}
/* the EMA set a resumed fit starts from, <weights>/ema/ (and its class table into ema_table, when not NULL), every file checked before the device is
 * opened; NULL when there is no such directory */
static float** load_ema_set(float* ema_table) {
	char path[512];
	struct stat sb;
	g_set = "ema";
	data_path(path, sizeof path, "");
	if (stat(path, &sb) != 0 || !S_ISDIR(sb.st_mode)) { g_set = ""; return NULL; }
	for (int t = 0; t < g_tensor_count; t++) {
		data_path(path, sizeof path, g_tensors[t].file);
		if (access(path, R_OK) != 0) { fprintf(stderr, "fit: the EMA set is incomplete: cannot open %s\n", path); exit(1); }
	}
	if (ema_table && !load_class_table(ema_table)) {
		data_path(path, sizeof path, "class_embedding.csv");
		fprintf(stderr, "fit: the EMA set is incomplete: cannot open %s\n", path);
		exit(1);
	}
	float** set = malloc(g_tensor_count * sizeof(float*));
	for (int t = 0; t < g_tensor_count; t++) set[t] = calloc((size_t)g_tensors[t].rows * g_tensors[t].cols, sizeof(float));
	swap_sets(set);
	load_parameters();
	swap_sets(set);
	g_set = "";
	return set;
}

/* ---- held-out evaluation: the variational bound in bits/dim (bla.h, "held-out evaluation"), for `eval` and for fit's BLA_UNET_EVAL_EVERY ------------- */
typedef struct Evaluator {
	size_t images;                       /* whole batches of the evaluation file's first records */
	int batch, K, T, *ts;                /* ts [K + 1]: bla_diffusion_eval_timesteps */
	float* d_data; int* d_labels;        /* the records, uploaded once; d_labels NULL: unconditional */
	double *d_out, *out;                 /* per batch: terms [K + 1][B], sqerr [K + 1][B], prior [B] */
	double prior, decoder, kl, *mse;     /* the last run: bits/dim of the three parts, eps MSE per timestep [K + 1] */
} Evaluator;
/* BLA_UNET_EVAL_STEPS: the number of KL terms, 0 .. T-1, default min(T - 1, 50) */
static int env_eval_steps(const char* verb, int T) {
	const char* v = getenv("BLA_UNET_EVAL_STEPS");
	if (!v || !*v) return T - 1 < 50 ? T - 1 : 50;
	char* end = NULL;
	const long k = strtol(v, &end, 10);
	if (*end || k < 0 || k > T - 1) { fprintf(stderr, "%s: BLA_UNET_EVAL_STEPS=%s; the bound has 0..%d KL terms (BLA_DIFFUSION_STEPS - 1)\n", verb, v, T - 1); exit(1); }
	return (int)k;
}
/* the evaluation file, BLA_CIFAR_EVAL_FILE (default <BLA_CIFAR_DIR>/test_batch.bin), read as read_training_set reads its files */
static float* read_eval_file(const char* verb, size_t* count, uint8_t** labels) {
	char path[512];
	snprintf(path, sizeof path, "%s/test_batch.bin", env_or("BLA_CIFAR_DIR", "data/cifar"));
	const char* file = env_or("BLA_CIFAR_EVAL_FILE", path);
	FILE* f = fopen(file, "rb");
	if (!f) { fprintf(stderr, "%s: cannot open %s: %s\n", verb, file, strerror(errno)); exit(1); }
	float* all = NULL;
	*count = 0;
	if (labels) *labels = NULL;
	read_records(f, &all, count, labels);
	fclose(f);
	for (size_t r = 0; labels && r < *count; r++)
		if ((*labels)[r] >= CLASSES) { fprintf(stderr, "%s: record %zu of %s has label %d; CIFAR-10 labels are 0..%d\n", verb, r, file, (*labels)[r], CLASSES - 1); exit(1); }
	return all;
}
/* after the device is open: uploads the first `images` records (a whole number of batches) and their labels (NULL: unconditional) */
static Evaluator eval_open(const bla_diffusion* diff, const float* data, const uint8_t* labels, size_t images, int batch, int K) {
	Evaluator ev; memset(&ev, 0, sizeof ev);
	ev.images = images; ev.batch = batch; ev.K = K; ev.T = bla_diffusion_steps(diff);
	ev.ts = malloc((K + 1) * sizeof(int));
	CHECK(bla_diffusion_eval_timesteps(diff, K, ev.ts));
	CHECK(bla_malloc((void**)&ev.d_data, images * IMAGE_FLOATS * sizeof(float)));
	CHECK(bla_memcpy_h2d(ev.d_data, data, images * IMAGE_FLOATS * sizeof(float), NULL));
	if (labels) {
		int* lab = malloc(images * sizeof(int));
		for (size_t r = 0; r < images; r++) lab[r] = labels[r];
		CHECK(bla_malloc((void**)&ev.d_labels, images * sizeof(int)));
		CHECK(bla_memcpy_h2d(ev.d_labels, lab, images * sizeof(int), NULL));
		CHECK(bla_stream_sync(NULL));
		free(lab);
	}
	const size_t doubles = (size_t)(2 * (K + 1) + 1) * batch;
	CHECK(bla_malloc((void**)&ev.d_out, doubles * sizeof(double)));
	ev.out = malloc(doubles * sizeof(double));
	ev.mse = malloc((K + 1) * sizeof(double));
	CHECK(bla_stream_sync(NULL));
	return ev;
}
/* One evaluation of the model's current weights: per batch bla_unet_evaluate_f32 (the batch that starts at record r draws at offset_base r F / 4, so every
 * record has its own noise whatever the batch size) and bla_diffusion_prior_kl_f32, the per-image doubles copied out once and summed here in record order.
 * Returns the bound in bits/dim: prior + decoder + (T - 1) / K x the K sampled KL terms, averaged over the images. */
static double eval_run(Evaluator* ev, bla_unet* net, const bla_diffusion* diff, unsigned long long seed, const float* d_table) {
	const int B = ev->batch, n = ev->K + 1;
	double prior = 0, decoder = 0, kl = 0;
	for (int i = 0; i < n; i++) ev->mse[i] = 0;
	double *terms = ev->out, *sqerr = ev->out + (size_t)n * B, *pri = ev->out + (size_t)2 * n * B;
	for (size_t r = 0; r < ev->images; r += B) {
		const float* x0 = ev->d_data + r * IMAGE_FLOATS;
		CHECK(bla_unet_evaluate_f32(net, diff, NULL, x0, ev->ts, n, seed, (unsigned long long)r * (IMAGE_FLOATS / 4), d_table, CLASSES,
		                            d_table ? ev->d_labels + r : NULL, ev->d_out, ev->d_out + (size_t)n * B));
		CHECK(bla_diffusion_prior_kl_f32(diff, NULL, x0, B, IMAGE_FLOATS, ev->d_out + (size_t)2 * n * B));
		CHECK(bla_memcpy_d2h(ev->out, ev->d_out, (size_t)(2 * n + 1) * B * sizeof(double), NULL));
		CHECK(bla_stream_sync(NULL));
		for (int b = 0; b < B; b++) {
			prior += pri[b]; decoder += terms[b];
			for (int i = 1; i < n; i++) kl += terms[(size_t)i * B + b];
			for (int i = 0; i < n; i++) ev->mse[i] += sqerr[(size_t)i * B + b];
		}
	}
	const double dims = (double)ev->images * IMAGE_FLOATS, bits = dims * log(2.0);
	ev->prior = prior / bits; ev->decoder = decoder / bits;
	ev->kl = ev->K ? kl * ((double)(ev->T - 1) / ev->K) / bits : 0.0;
	for (int i = 0; i < n; i++) ev->mse[i] /= dims;
	return ev->prior + ev->decoder + ev->kl;
}
static void eval_close(Evaluator* ev) {
	CHECK(bla_free(ev->d_data)); CHECK(bla_free(ev->d_labels)); CHECK(bla_free(ev->d_out));
	free(ev->ts); free(ev->out); free(ev->mse);
}

/* `eval [<images>]`: the saved set (BLA_UNET_EVAL_EMA=1: the set below ema/) on the evaluation file's first <images> records (default all), the last partial
 * batch dropped; BLA_UNET_BATCH (default 64), BLA_UNET_EVAL_STEPS, BLA_UNET_CLASSES=1: every image with its own label's row, no label dropout */
static void eval(const char* images_arg) {
	if (env_flag("BLA_UNET_EVAL_EMA")) g_set = "ema";
	const Objective obj = resolve_objective("eval", 1);
	const int classes = env_flag("BLA_UNET_CLASSES"), T = env_steps(), K = env_eval_steps("eval", T);
	const int batch = atoi(env_or("BLA_UNET_BATCH", "64"));
	if (batch < 1) { fprintf(stderr, "eval: BLA_UNET_BATCH must be >= 1\n"); exit(1); }
	long want = -1;
	if (images_arg) {
		char* end = NULL;
		want = strtol(images_arg, &end, 10);
		if (*end || want < 1) { fprintf(stderr, "eval: %s images; the number of images is a whole number >= 1\n", images_arg); exit(1); }
	}
	size_t records = 0;
	uint8_t* labels = NULL;
	float* data = read_eval_file("eval", &records, classes ? &labels : NULL);
	if (want > 0 && (size_t)want < records) records = (size_t)want;
	const size_t images = records / batch * batch;
	if (!images) { fprintf(stderr, "eval: %zu records, fewer than one batch of %d\n", records, batch); exit(1); }
	float* table = NULL;
	if (classes) {
		table = malloc((size_t)(CLASSES + 1) * TIME_EMBED_DIM * sizeof(float));
		if (!load_class_table(table)) {
			char path[512];
			data_path(path, sizeof path, "class_embedding.csv");
			fprintf(stderr, "eval: cannot open %s (run `fit` with BLA_UNET_CLASSES=1 first)\n", path);
			exit(1);
		}
	}
	load_parameters();
	const unsigned long long seed = env_seed();
	Inputs in = inputs_alloc(1);
	Device dv = device_open(batch, in.drop_per_image);
	device_set_params(&dv);
	bla_diffusion* diff = open_diffusion(&obj, T);
	float* d_table = NULL;
	if (classes) {
		CHECK(bla_malloc((void**)&d_table, (size_t)(CLASSES + 1) * TIME_EMBED_DIM * sizeof(float)));
		CHECK(bla_memcpy_h2d(d_table, table, (size_t)(CLASSES + 1) * TIME_EMBED_DIM * sizeof(float), NULL));
	}
	Evaluator ev = eval_open(diff, data, labels, images, batch, K);
	free(data); free(labels);
	const double total = eval_run(&ev, dv.net, diff, seed, d_table);
	if (!isfinite(total)) { fprintf(stderr, "eval: the bound is not finite (%f bits/dim)\n", total); exit(1); }
	printf("eval: %zu images, %d steps, %d of %d KL terms\n", images, T, K, T - 1);
	printf("Bits/dim: %.6f (prior %.6f, decoder %.6f, KL %.6f)\n", total, ev.prior, ev.decoder, ev.kl);
	printf("Eps MSE by timestep:");
	for (int i = 0; i <= K; i++) printf(" t=%d %.6f", ev.ts[i], ev.mse[i]);
	printf("\n");
	eval_close(&ev);
	if (classes) { CHECK(bla_free(d_table)); free(table); }
	CHECK(bla_diffusion_destroy(diff));
	inputs_free(&in); device_close(&dv);
}

static void fit(int epochs, int batch) {
	if (batch < 1 || epochs < 1) { fprintf(stderr, "fit: epochs and batch must be >= 1\n"); exit(1); }
	const Objective obj = resolve_objective("fit", env_flag("BLA_UNET_RESUME"));
	const double ema_decay = env_ema_decay();
	const int shuffle = env_fit_flag("BLA_UNET_SHUFFLE"), flip = env_fit_flag("BLA_UNET_FLIP"), gather = shuffle || flip;
	const double clip_norm = env_clip_norm();
	const long warmup = env_warmup();
	const long eval_every = env_eval_every();
	const int classes = env_flag("BLA_UNET_CLASSES");
	size_t records = 0;
	uint8_t* labels = NULL;
	float* data = read_training_set(&records, classes ? &labels : NULL);
	const size_t per_epoch = records / batch;                                                   /* the last partial batch is dropped */
	if (per_epoch == 0) { fprintf(stderr, "fit: %zu records, fewer than one batch of %d\n", records, batch); exit(1); }
	if (shuffle && records > ((size_t)1 << 20)) { fprintf(stderr, "fit: BLA_UNET_SHUFFLE=1 takes at most 2^20 records, not %zu\n", records); exit(1); }
	float* table = NULL;
	const double p_uncond = atof(env_or("BLA_UNET_UNCOND", "0.1"));
	if (classes) {
		for (size_t r = 0; r < records; r++)
			if (labels[r] >= CLASSES) { fprintf(stderr, "fit: record %zu has label %d; CIFAR-10 labels are 0..%d\n", r, labels[r], CLASSES - 1); exit(1); }
		if (!(p_uncond >= 0 && p_uncond <= 1)) { fprintf(stderr, "fit: BLA_UNET_UNCOND must lie in [0, 1]\n"); exit(1); }
		table = calloc((size_t)(CLASSES + 1) * TIME_EMBED_DIM, sizeof(float));
		if (env_flag("BLA_UNET_RESUME")) (void)load_class_table(table);
	}
	/* BLA_UNET_EVAL_EVERY: the held-out records, read and checked before the device is opened */
	float* eval_data = NULL; uint8_t* eval_labels = NULL; size_t eval_images = 0; int eval_K = 0;
	if (eval_every) {
		eval_K = env_eval_steps("fit", env_steps());
		const char* v = getenv("BLA_UNET_EVAL_IMAGES");
		char* end = NULL;
		const long want = v && *v ? strtol(v, &end, 10) : batch;
		if ((end && *end) || want < batch) { fprintf(stderr, "fit: BLA_UNET_EVAL_IMAGES=%s; the evaluation takes a whole number of images, at least one batch of %d\n", v ? v : "", batch); exit(1); }
		size_t held = 0;
		eval_data = read_eval_file("fit", &held, classes ? &eval_labels : NULL);
		eval_images = (size_t)want / batch * batch;
		if (held < eval_images) { fprintf(stderr, "fit: the evaluation file holds %zu records, fewer than the %zu asked for\n", held, eval_images); exit(1); }
	}
	if (env_flag("BLA_UNET_RESUME")) load_parameters(); else draw_parameters("unit");
	const size_t table_floats = (size_t)(CLASSES + 1) * TIME_EMBED_DIM;
	float* ema_table = NULL;   /* BLA_UNET_EMA: the average's class table (host), and the resumed EMA set (NULL: the average starts from the parameters) */
	float** ema_set = NULL;
	if (ema_decay > 0) {
		if (classes) { ema_table = malloc(table_floats * sizeof(float)); memcpy(ema_table, table, table_floats * sizeof(float)); }
		if (env_flag("BLA_UNET_RESUME")) ema_set = load_ema_set(ema_table);
	}
	const unsigned long long seed = env_seed();
	const double lr = atof(env_or("BLA_ADAM_LR", "2e-4"));
	int log_every = atoi(env_or("BLA_UNET_LOG_EVERY", "50"));
	if (log_every < 1) log_every = 1;
	Inputs in = inputs_alloc(1);                                                                /* only for the dropout layout */
	Device dv = device_open(batch, in.drop_per_image);
	device_set_params(&dv);
	bla_diffusion* diff = open_diffusion(&obj, env_steps());
	/* a shuffled epoch draws from every record; otherwise the last partial batch is never seen and is not uploaded */
	const size_t params = bla_unet_param_count(dv.net), drops = bla_unet_dropout_count(dv.net), used = shuffle ? records : per_epoch * batch;
	float *d_data, *d_m, *d_v; int* d_t; double* d_loss;
	CHECK(bla_malloc((void**)&d_data, used * IMAGE_FLOATS * sizeof(float)));
	CHECK(bla_memcpy_h2d(d_data, data, used * IMAGE_FLOATS * sizeof(float), NULL));
	CHECK(bla_malloc((void**)&d_m, params * sizeof(float))); CHECK(bla_memset(d_m, 0, params * sizeof(float), NULL));
	CHECK(bla_malloc((void**)&d_v, params * sizeof(float))); CHECK(bla_memset(d_v, 0, params * sizeof(float), NULL));
	CHECK(bla_malloc((void**)&d_t, batch * sizeof(int)));
	CHECK(bla_malloc((void**)&d_loss, sizeof(double))); CHECK(bla_memset(d_loss, 0, sizeof(double), NULL));
	float *d_ema = NULL, *d_ema_table = NULL;
	if (ema_decay > 0) {   /* device_set_params reuses the bucket's host image: each upload is waited for before the next */
		CHECK(bla_malloc((void**)&d_ema, params * sizeof(float)));
		if (ema_set) { CHECK(bla_stream_sync(NULL)); swap_sets(ema_set); device_set_params(&dv); }
		CHECK(bla_memcpy_d2d(d_ema, bla_unet_params(dv.net), params * sizeof(float), NULL));
		if (ema_set) { CHECK(bla_stream_sync(NULL)); swap_sets(ema_set); device_set_params(&dv); }
		if (classes) {
			CHECK(bla_malloc((void**)&d_ema_table, table_floats * sizeof(float)));
			CHECK(bla_memcpy_h2d(d_ema_table, ema_table, table_floats * sizeof(float), NULL));
		}
	}
	/* an objective in force: the regression target, the seed of the backward pass, the per-image weights and losses (one row per pass between two logged
	 * lines, summed on the host in order), and the assembled x0 batch where the noising launch gathers it */
	float *d_target = NULL, *d_g = NULL, *d_weight = NULL, *d_x0 = NULL; double* d_losses = NULL; double* losses = NULL;
	if (obj.active) {
		CHECK(bla_malloc((void**)&d_target, (size_t)batch * IMAGE_FLOATS * sizeof(float)));
		CHECK(bla_malloc((void**)&d_g, (size_t)batch * IMAGE_FLOATS * sizeof(float)));
		CHECK(bla_malloc((void**)&d_weight, batch * sizeof(float)));
		if (gather) CHECK(bla_malloc((void**)&d_x0, (size_t)batch * IMAGE_FLOATS * sizeof(float)));
		CHECK(bla_malloc((void**)&d_losses, (size_t)log_every * batch * sizeof(double)));
		losses = malloc((size_t)log_every * batch * sizeof(double));
	}
	unsigned int *d_index = NULL, *d_keys = NULL;   /* BLA_UNET_SHUFFLE / BLA_UNET_FLIP: the epoch's record order (0, 1, 2, ... without shuffling) */
	if (gather) {
		CHECK(bla_malloc((void**)&d_index, used * sizeof(unsigned int)));
		if (shuffle) {
			CHECK(bla_malloc((void**)&d_keys, used * sizeof(unsigned int)));
		} else {
			unsigned int* order = malloc(used * sizeof(unsigned int));
			for (size_t r = 0; r < used; r++) order[r] = (unsigned int)r;
			CHECK(bla_memcpy_h2d(d_index, order, used * sizeof(unsigned int), NULL));
			CHECK(bla_stream_sync(NULL));
			free(order);
		}
	}
	double *d_sumsq = NULL, *d_partials = NULL; float *d_scale = NULL, *d_norm = NULL;   /* BLA_ADAM_CLIP_NORM */
	if (clip_norm > 0) {
		CHECK(bla_malloc((void**)&d_sumsq, sizeof(double))); CHECK(bla_malloc((void**)&d_partials, BLA_SUMSQ_SCRATCH_DOUBLES * sizeof(double)));
		CHECK(bla_malloc((void**)&d_scale, sizeof(float))); CHECK(bla_malloc((void**)&d_norm, sizeof(float)));
	}
	float *d_table = NULL, *d_gtable = NULL, *d_tm = NULL, *d_tv = NULL, *d_dtemb = NULL; int *d_labels = NULL, *d_rows = NULL, *d_batch_labels = NULL;
	if (classes) {
		int* lab = malloc(used * sizeof(int));
		for (size_t r = 0; r < used; r++) lab[r] = labels[r];
		CHECK(bla_malloc((void**)&d_labels, used * sizeof(int)));
		CHECK(bla_memcpy_h2d(d_labels, lab, used * sizeof(int), NULL));
		CHECK(bla_malloc((void**)&d_table, table_floats * sizeof(float)));
		CHECK(bla_memcpy_h2d(d_table, table, table_floats * sizeof(float), NULL));
		CHECK(bla_malloc((void**)&d_gtable, table_floats * sizeof(float)));
		CHECK(bla_malloc((void**)&d_tm, table_floats * sizeof(float))); CHECK(bla_memset(d_tm, 0, table_floats * sizeof(float), NULL));
		CHECK(bla_malloc((void**)&d_tv, table_floats * sizeof(float))); CHECK(bla_memset(d_tv, 0, table_floats * sizeof(float), NULL));
		CHECK(bla_malloc((void**)&d_dtemb, (size_t)batch * TIME_EMBED_DIM * sizeof(float)));
		CHECK(bla_malloc((void**)&d_rows, batch * sizeof(int)));
		if (gather) CHECK(bla_malloc((void**)&d_batch_labels, batch * sizeof(int)));
		CHECK(bla_stream_sync(NULL));
		free(lab);
	}
	Evaluator ev; memset(&ev, 0, sizeof ev);
	if (eval_every) { ev = eval_open(diff, eval_data, eval_labels, eval_images, batch, eval_K); free(eval_data); free(eval_labels); }
	CHECK(bla_stream_sync(NULL));
	free(data); free(labels);
	printf("fit: %zu records, %zu passes of %d per epoch, %d epochs\n", records, per_epoch, batch, epochs);
	const size_t passes = per_epoch * epochs;
	size_t logged = 0;
	for (size_t pass = 0; pass < passes; pass++) {
		const size_t k = pass % per_epoch;
		const int* pass_labels = classes ? d_labels + k * batch : NULL;
		const float* x0 = d_data + k * batch * IMAGE_FLOATS;   /* the pass's clean images (read only with an objective in force) */
		if (gather) {   /* index, flips and labels inside the noising launch; a shuffled epoch starts with its permutation (Philox offsets: bla.h) */
			if (shuffle && k == 0)
				CHECK(bla_rand_permutation_u32(NULL, d_index, d_keys, records, seed, ((unsigned long long)(pass / per_epoch) << 32) + (1ull << 31)));
			CHECK(bla_diffusion_noise_gather_f32(diff, NULL, d_data, used, d_index + k * batch, flip, IMAGE_SIDE, d_labels, d_batch_labels, batch, IMAGE_FLOATS,
			                                     TIME_EMBED_DIM, seed, pass, d_t, dv.noise, dv.x, dv.temb, d_x0));
			pass_labels = d_batch_labels;
			x0 = d_x0;
		} else {
			CHECK(bla_diffusion_noise_f32(diff, NULL, d_data + k * batch * IMAGE_FLOATS, batch, IMAGE_FLOATS, TIME_EMBED_DIM, seed, pass, d_t, dv.noise, dv.x, dv.temb));
		}
		if (classes)   /* the label dropout's Philox blocks start at (pass << 32) + 2^31, behind the dropout decisions' (bla.h) */
			CHECK(bla_class_embedding_f32(NULL, d_table, CLASSES, pass_labels, batch, TIME_EMBED_DIM, (float)p_uncond, seed,
			                              ((unsigned long long)pass << 32) + (1ull << 31), d_rows, dv.temb));
		CHECK(bla_rand_bernoulli_u8(NULL, dv.drop, drops, DROPOUT_RATE, seed, (unsigned long long)pass << 32));
		if (obj.active) {   /* target and weights of the objective, forward, the weighted loss with its gradient, backward from that gradient */
			CHECK(bla_diffusion_target_f32(diff, NULL, x0, dv.noise, d_t, 0, batch, IMAGE_FLOATS, d_target, d_weight));
			CHECK(bla_unet_forward_f32(dv.net, NULL, dv.x, dv.temb, dv.drop));
			CHECK(bla_diffusion_loss_f32(NULL, bla_unet_output(dv.net), d_target, d_weight, batch, IMAGE_FLOATS, d_g, d_losses + (pass - logged) * batch));
			CHECK(bla_unet_backward_from_f32(dv.net, NULL, d_g));
		} else {
			CHECK(bla_unet_forward_f32(dv.net, NULL, dv.x, dv.temb, dv.drop));
			CHECK(bla_unet_backward_f32(dv.net, NULL, dv.noise));
		}
		if (classes) {
			CHECK(bla_unet_embedding_grad_f32(dv.net, NULL, d_dtemb));
			CHECK(bla_class_embedding_grad_f32(NULL, d_dtemb, d_rows, batch, CLASSES, TIME_EMBED_DIM, d_gtable));
		}
		if (!obj.active) CHECK(bla_mse_accumulate_f32(NULL, bla_unet_output(dv.net), dv.noise, (size_t)batch * IMAGE_FLOATS, d_loss));
		const float pass_lr = warmup ? (float)(lr * fmin(1.0, (double)(pass + 1) / (double)warmup)) : (float)lr;
		if (clip_norm > 0) {   /* the global norm of the mean gradient over both buckets, the clipping coefficient and Adam's grad_scale all stay on the device */
			CHECK(bla_memset(d_sumsq, 0, sizeof(double), NULL));
			CHECK(bla_sumsq_accumulate_f32(NULL, bla_unet_grads(dv.net), params, d_sumsq, d_partials));
			if (classes) CHECK(bla_sumsq_accumulate_f32(NULL, d_gtable, table_floats, d_sumsq, d_partials));
			CHECK(bla_clip_scale_f32(NULL, d_sumsq, 1.0f / batch, (float)clip_norm, d_scale, d_norm));
			CHECK(bla_adam_scaled_f32(NULL, bla_unet_params(dv.net), bla_unet_grads(dv.net), d_m, d_v, params, pass_lr, 0.9f, 0.999f, 1e-8f, 0.f, d_scale, (int)(pass + 1)));
			if (classes)
				CHECK(bla_adam_scaled_f32(NULL, d_table, d_gtable, d_tm, d_tv, table_floats, pass_lr, 0.9f, 0.999f, 1e-8f, 0.f, d_scale, (int)(pass + 1)));
		} else {
			CHECK(bla_adam_f32(NULL, bla_unet_params(dv.net), bla_unet_grads(dv.net), d_m, d_v, params, pass_lr, 0.9f, 0.999f, 1e-8f, 0.f, 1.0f / batch, (int)(pass + 1)));
			if (classes)
				CHECK(bla_adam_f32(NULL, d_table, d_gtable, d_tm, d_tv, table_floats, pass_lr, 0.9f, 0.999f, 1e-8f, 0.f, 1.0f / batch, (int)(pass + 1)));
		}
		if (ema_decay > 0) {   /* the warm-up keeps the early average from holding on to the initial draw */
			const float decay = (float)fmin(ema_decay, (1.0 + pass) / (10.0 + pass));
			CHECK(bla_ema_f32(NULL, d_ema, bla_unet_params(dv.net), params, decay));
			if (classes) CHECK(bla_ema_f32(NULL, d_ema_table, d_table, table_floats, decay));
		}
		if ((pass + 1) % log_every == 0 || pass + 1 == passes) {
			double sum = 0;
			float norm = 0;
			if (obj.active) CHECK(bla_memcpy_d2h(losses, d_losses, (pass + 1 - logged) * batch * sizeof(double), NULL));
			else CHECK(bla_memcpy_d2h(&sum, d_loss, sizeof sum, NULL));
			if (clip_norm > 0) CHECK(bla_memcpy_d2h(&norm, d_norm, sizeof norm, NULL));
			CHECK(bla_memset(d_loss, 0, sizeof(double), NULL));
			CHECK(bla_stream_sync(NULL));
			if (obj.active) for (size_t i = 0; i < (pass + 1 - logged) * batch; i++) sum += losses[i];   /* the mean weighted loss */
			printf("Pass %zu:\tAvg loss: %f\n", pass, sum / ((double)(pass + 1 - logged) * batch * IMAGE_FLOATS));
			if (clip_norm > 0) printf("Grad norm: %f\n", norm);
			fflush(stdout);
			logged = pass + 1;
		}
		if (eval_every && ((pass + 1) % (size_t)eval_every == 0 || pass + 1 == passes)) {   /* the live weights on the held-out records: a fixed seed and K */
			printf("Held-out bits/dim: %.6f\n", eval_run(&ev, dv.net, diff, seed, d_table));
			fflush(stdout);
		}
	}
	if (eval_every) eval_close(&ev);
	device_get_params(&dv);
	save_parameters();
	if (obj.active) save_objective(&obj); else remove_objective();
	if (ema_decay > 0) {   /* the average as a second complete set below ema/: tensors the device model does not use keep the values just written */
		CHECK(bla_memcpy_d2d(bla_unet_params(dv.net), d_ema, params * sizeof(float), NULL));
		device_get_params(&dv);
		g_set = "ema";
		save_parameters();
		if (obj.active) save_objective(&obj); else remove_objective();
		if (classes) {
			CHECK(bla_memcpy_d2h(ema_table, d_ema_table, table_floats * sizeof(float), NULL));
			CHECK(bla_stream_sync(NULL));
			save_class_table(ema_table);
			CHECK(bla_free(d_ema_table));
			free(ema_table);
		}
		g_set = "";
		CHECK(bla_free(d_ema));
		if (ema_set) { for (int t = 0; t < g_tensor_count; t++) free(ema_set[t]); free(ema_set); }
	}
	if (classes) {
		CHECK(bla_memcpy_d2h(table, d_table, table_floats * sizeof(float), NULL));
		CHECK(bla_stream_sync(NULL));
		save_class_table(table);
		CHECK(bla_free(d_labels)); CHECK(bla_free(d_table)); CHECK(bla_free(d_gtable)); CHECK(bla_free(d_tm)); CHECK(bla_free(d_tv));
		CHECK(bla_free(d_dtemb)); CHECK(bla_free(d_rows)); CHECK(bla_free(d_batch_labels));
		free(table);
	}
	if (gather) { CHECK(bla_free(d_index)); CHECK(bla_free(d_keys)); }
	if (clip_norm > 0) { CHECK(bla_free(d_sumsq)); CHECK(bla_free(d_partials)); CHECK(bla_free(d_scale)); CHECK(bla_free(d_norm)); }
	if (obj.active) { CHECK(bla_free(d_target)); CHECK(bla_free(d_g)); CHECK(bla_free(d_weight)); CHECK(bla_free(d_x0)); CHECK(bla_free(d_losses)); free(losses); }
	CHECK(bla_free(d_data)); CHECK(bla_free(d_m)); CHECK(bla_free(d_v)); CHECK(bla_free(d_t)); CHECK(bla_free(d_loss));
	CHECK(bla_diffusion_destroy(diff));
	inputs_free(&in); device_close(&dv);
}

static void sample(int count, const char* dir) {
	int batch = atoi(env_or("BLA_UNET_BATCH", "16"));
	if (batch > count) batch = count;
	if (batch < 1) return;
	const Objective obj = resolve_objective("sample", 1);
	/* BLA_UNET_SAMPLE_STEPS=S: DDIM with S steps, BLA_UNET_ETA, BLA_UNET_CLIP; checked before the device is opened */
	const char* steps_env = getenv("BLA_UNET_SAMPLE_STEPS");
	const int ddim = steps_env && *steps_env;
	int sample_steps = 0;
	if (ddim) {
		char* end = NULL;
		const long s = strtol(steps_env, &end, 10);
		const int T = env_steps();
		if (*end || s < 1 || s > T) { fprintf(stderr, "sample: BLA_UNET_SAMPLE_STEPS=%s; DDIM takes 1..%d steps (BLA_DIFFUSION_STEPS)\n", steps_env, T); exit(1); }
		sample_steps = (int)s;
	}
	const char* eta_env = env_or("BLA_UNET_ETA", "0");
	char* eta_end = NULL;
	const double eta = strtod(eta_env, &eta_end);
	if (*eta_end || !(eta >= 0 && eta <= 1)) { fprintf(stderr, "sample: BLA_UNET_ETA=%s; eta must lie in [0, 1]\n", eta_env); exit(1); }
	const int clip = env_flag("BLA_UNET_CLIP");
	/* BLA_UNET_SAMPLER=dpmpp: DPM-Solver++(2M) over BLA_UNET_SAMPLE_STEPS steps spaced by BLA_UNET_SPACING; checked before the device is opened */
	const char* sampler_env = getenv("BLA_UNET_SAMPLER");
	int dpmpp = 0, spacing = BLA_SPACING_LOGSNR;
	if (sampler_env && *sampler_env) {
		if (strcmp(sampler_env, "dpmpp") == 0) dpmpp = 1;
		else if (strcmp(sampler_env, "ddim") != 0) { fprintf(stderr, "sample: BLA_UNET_SAMPLER=%s; the samplers are ddim and dpmpp\n", sampler_env); exit(1); }
		const char* spacing_env = env_or("BLA_UNET_SPACING", "logsnr");
		if (strcmp(spacing_env, "trailing") == 0) spacing = BLA_SPACING_TRAILING;
		else if (strcmp(spacing_env, "logsnr") != 0) { fprintf(stderr, "sample: BLA_UNET_SPACING=%s; the spacings are logsnr and trailing\n", spacing_env); exit(1); }
		if (!ddim) { fprintf(stderr, "sample: BLA_UNET_SAMPLER=%s needs BLA_UNET_SAMPLE_STEPS\n", sampler_env); exit(1); }
		if (dpmpp && eta != 0) { fprintf(stderr, "sample: BLA_UNET_ETA=%s; BLA_UNET_SAMPLER=dpmpp is deterministic and takes no eta\n", eta_env); exit(1); }
	}
	/* BLA_UNET_CLASS=k: guided sampling of class k with the table fit wrote; both checked before the device is opened */
	const char* class_env = getenv("BLA_UNET_CLASS");
	const int guided = class_env && *class_env;
	int klass = 0;
	float guidance = 0.f, *table = NULL;
	if (guided) {
		char* end = NULL;
		const long k = strtol(class_env, &end, 10);
		if (*end || k < 0 || k >= CLASSES) { fprintf(stderr, "sample: BLA_UNET_CLASS=%s; the classes are 0..%d\n", class_env, CLASSES - 1); exit(1); }
		klass = (int)k;
		guidance = (float)atof(env_or("BLA_UNET_GUIDANCE", "3"));
		table = malloc((size_t)(CLASSES + 1) * TIME_EMBED_DIM * sizeof(float));
		if (!load_class_table(table)) {
			char path[512];
			data_path(path, sizeof path, "class_embedding.csv");
			fprintf(stderr, "sample: cannot open %s (run `fit` with BLA_UNET_CLASSES=1 first)\n", path);
			exit(1);
		}
	}
	load_parameters();
	if (mkdir(dir, 0777) != 0 && errno != EEXIST) { fprintf(stderr, "cannot make %s: %s\n", dir, strerror(errno)); exit(1); }
	const unsigned long long seed = env_seed();
	Inputs in = inputs_alloc(1);
	Device dv = device_open(guided ? 2 * batch : batch, in.drop_per_image);   /* guided: n conditioned images + their n null-class copies */
	device_set_params(&dv);
	bla_diffusion* diff = open_diffusion(&obj, env_steps());
	float* d_table = NULL; int* d_labels = NULL;
	if (guided) {
		int* lab = malloc(batch * sizeof(int));
		for (int b = 0; b < batch; b++) lab[b] = klass;
		CHECK(bla_malloc((void**)&d_table, (size_t)(CLASSES + 1) * TIME_EMBED_DIM * sizeof(float)));
		CHECK(bla_memcpy_h2d(d_table, table, (size_t)(CLASSES + 1) * TIME_EMBED_DIM * sizeof(float), NULL));
		CHECK(bla_malloc((void**)&d_labels, batch * sizeof(int)));
		CHECK(bla_memcpy_h2d(d_labels, lab, batch * sizeof(int), NULL));
		CHECK(bla_stream_sync(NULL));
		free(lab);
	}
	float* x = malloc((size_t)batch * IMAGE_FLOATS * sizeof(float));
	uint8_t planes[IMAGE_FLOATS];
	int done = 0;
	for (unsigned long long k = 0; done < count; k++) {
		CHECK(bla_rand_normal_f32(NULL, dv.x, (size_t)batch * IMAGE_FLOATS, 0.f, 1.f, seed + k, 0));   /* x_T */
		if (guided && dpmpp)
			CHECK(bla_unet_sample_guided_dpmpp_f32(dv.net, diff, NULL, dv.x, d_table, CLASSES, d_labels, guidance, sample_steps, spacing, clip));
		else if (dpmpp) CHECK(bla_unet_sample_dpmpp_f32(dv.net, diff, NULL, dv.x, sample_steps, spacing, clip));
		else if (guided && ddim)
			CHECK(bla_unet_sample_guided_ddim_f32(dv.net, diff, NULL, dv.x, d_table, CLASSES, d_labels, guidance, sample_steps, (float)eta, clip, seed + k));
		else if (guided) CHECK(bla_unet_sample_guided_f32(dv.net, diff, NULL, dv.x, d_table, CLASSES, d_labels, guidance, seed + k));
		else if (ddim) CHECK(bla_unet_sample_ddim_f32(dv.net, diff, NULL, dv.x, sample_steps, (float)eta, clip, seed + k));
		else CHECK(bla_unet_sample_f32(dv.net, diff, NULL, dv.x, seed + k));
		CHECK(bla_memcpy_d2h(x, dv.x, (size_t)batch * IMAGE_FLOATS * sizeof(float), NULL));
		CHECK(bla_stream_sync(NULL));
		for (int b = 0; b < batch && done < count; b++, done++) {
			for (int i = 0; i < IMAGE_FLOATS; i++) {                                            /* the inverse of load_example's (p - 127.5) / 127.5 */
				const double v = round(((double)x[(size_t)b * IMAGE_FLOATS + i] + 1.0) * 127.5);
				planes[i] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
			}
			BMPData img = {IMAGE_SIDE, IMAGE_SIDE, planes, planes + IMAGE_SIDE * IMAGE_SIDE, planes + 2 * IMAGE_SIDE * IMAGE_SIDE};
			char path[512];
			snprintf(path, sizeof path, "%s/sample_%04d.bmp", dir, done);
			write_bmp_data(path, &img);
		}
	}
	printf("Wrote %d samples to %s\n", count, dir);
	free(x);
	if (guided) { CHECK(bla_free(d_table)); CHECK(bla_free(d_labels)); free(table); }
	CHECK(bla_diffusion_destroy(diff));
	inputs_free(&in); device_close(&dv);
}

int main(int argc, char** argv) {
	rng_seed(42);                                                                               /* srand(42), :1941 */
	if (argc < 2) {
		printf("Please supply an argument, options:\n\trun [<num samples> (default 1)]\n\ttrain <num epochs>\n\tinit\n");
		exit(1);
	}
	products_from_env();   /* before any sub-command opens the device: a bad value stops every one of them */
	attention_from_env();
	heads_from_env(g_attention);
	plan_model();
	if (strncmp(argv[1], "run", 3) == 0) {
		run(argc < 3 ? 1 : atoi(argv[2]));
	} else if (strncmp(argv[1], "train", 5) == 0) {
		if (argc < 3) {
			printf("Please supply a number of epochs, usage:\n\ttrain <num_epochs>\n");
			exit(1);
		}
		train(atoi(argv[2]), argc < 4 ? 1 : atoi(argv[3]));
	} else if (strncmp(argv[1], "init", 4) == 0) {
		init();
	} else if (strcmp(argv[1], "draws") == 0 && argc >= 4) {
		draws(atoi(argv[2]), argv[3]);
	} else if (strcmp(argv[1], "fit") == 0) {
		if (argc < 3) {
			printf("Please supply a number of epochs, usage:\n\tfit <num_epochs> [<batch> (default 64)]\n");
			exit(1);
		}
		fit(atoi(argv[2]), argc < 4 ? 64 : atoi(argv[3]));
	} else if (strcmp(argv[1], "eval") == 0) {
		eval(argc < 3 ? NULL : argv[2]);
	} else if (strcmp(argv[1], "sample") == 0) {
		sample(argc < 3 ? 1 : atoi(argv[2]), argc < 4 ? "data/cifar_unet_samples" : argv[3]);
	} else {
		printf("Unrecognized argument, options:\n\trun [<num samples> (default 1)]\n\ttrain <num epochs>\n\tinit\n");
		exit(1);
	}
	return 0;
}
