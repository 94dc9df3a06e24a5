// CCV_16F tensors on rows whose kernels compute in fp32: the command runs on fp32 IMAGES of its half-precision tensors.
//
// The reference's GPU rows register CCV_32F | CCV_16F (e.g. lib/nnc/cmd/convolution/gpu/ccv_nnc_conv_gpu_cudnn.cu:478-500,
// lib/nnc/cmd/sgd/gpu/ccv_nnc_sgd_gpu_ref.cu:13-100 with its mixed fp16 / fp32 variants) and its trainers store activations and
// gradients in half precision (test/int/nnc/cifar.tests.c:473).  Rows with a native half-precision kernel (the contraction core:
// GEMM and convolution on v_mfma_f32_32x32x16_f16, cmd_gemm.cpp / cmd_conv.cpp) handle CCV_16F themselves; every other row
// takes this route, so that a half-precision graph never meets a row that cannot run it:
//   1. every distinct CCV_16F tensor of the command gets an fp32 image in the stream's staging arena (device_rt.cpp; separate
//      from the workspace, which the command underneath may grow and thereby move);
//   2. inputs are converted up (exact); outputs that are accumulated into or alias an input are converted up too;
//   3. the fp32 exec function runs on shadow tensor structs (same shape / strides / view flags, datatype CCV_32F);
//   4. outputs are converted down (round to nearest even, as the reference's ccv_float_to_half_precision does) -- a dense tensor as one
//      run, a VIEW element by element through its strides: what lies between a view's rows is not this command's to write.
// Storage is half precision, arithmetic fp32: at least the accuracy the reference's own half-precision kernels have (they
// accumulate in fp32 as well), so its GPU-vs-CPU tolerances hold.  Cost: one extra read + write of each half tensor -- this is
// the coverage path, not the fast one.
#include "common.h"

namespace nnc {

typedef _Float16 half_t;
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// n elements, contiguous.  Four per thread where the alignment allows (8-byte / 16-byte accesses).
static __global__ void __launch_bounds__(256) half_up_kernel(const half_t* __restrict__ in, float* __restrict__ out, const size_t n, const int vec)
{
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	if (vec) {
		const size_t n4 = n >> 2;
		for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
			const half4_t v = ((const half4_t*)in)[i];
			((f32x4_t*)out)[i] = f32x4_t{ (float)v[0], (float)v[1], (float)v[2], (float)v[3] };
		}
		for (size_t i = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (float)in[i];
	} else
		for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (float)in[i];
}
static __global__ void __launch_bounds__(256) half_down_kernel(const float* __restrict__ in, half_t* __restrict__ out, const size_t n, const int vec)
{
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	if (vec) {
		const size_t n4 = n >> 2;
		for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
			const f32x4_t v = ((const f32x4_t*)in)[i];
			((half4_t*)out)[i] = half4_t{ (half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3] };
		}
		for (size_t i = (n4 << 2) + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (half_t)in[i];
	} else
		for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (half_t)in[i];
}

// A VIEW's elements only, from the fp32 image of its span back to the half tensor: the gaps between a view's rows belong to somebody else (sibling
// views of one parent -- channel-concatenated branches the host may run on other streams) and are never written.  One thread per element.
struct view_geom_t { int nd; int dim[CCV_NNC_MAX_DIM_ALLOC]; int stride[CCV_NNC_MAX_DIM_ALLOC]; };
static __global__ void __launch_bounds__(256) half_down_view_kernel(const float* __restrict__ in, half_t* __restrict__ out, const size_t n, const view_geom_t g)
{
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		size_t r = i, off = 0;
		for (int d = g.nd - 1; d >= 0; d--) { off += (r % (size_t)g.dim[d]) * (size_t)g.stride[d]; r /= (size_t)g.dim[d]; }
		out[off] = (half_t)in[off];
	}
}
static int float_to_half_view(const float* image, void* half, const ccv_nnc_tensor_t* t, ccv_nnc_stream_context_t* ctx)
{
	view_geom_t g;
	int st[CCV_NNC_MAX_DIM_ALLOC];
	tensor_strides(t, st);
	g.nd = tensor_nd(t->info.dim);
	size_t n = 1;
	for (int i = 0; i < g.nd; i++) { g.dim[i] = t->info.dim[i]; g.stride[i] = st[i]; n *= (size_t)t->info.dim[i]; }
	if (!n || !g.nd) return CCV_NNC_EXEC_SUCCESS;
	hipLaunchKernelGGL(half_down_view_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream_of(ctx), image, (half_t*)half, n, g);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

int half_to_float(const void* in, float* out, size_t n, ccv_nnc_stream_context_t* ctx)
{
	if (!n) return CCV_NNC_EXEC_SUCCESS;
	const int vec = (((uintptr_t)in & 7) == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
	hipLaunchKernelGGL(half_up_kernel, dim3(grid_for(vec ? (n + 3) / 4 : n, 256)), dim3(256), 0, stream_of(ctx), (const half_t*)in, out, n, vec);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}
int float_to_half(const float* in, void* out, size_t n, ccv_nnc_stream_context_t* ctx)
{
	if (!n) return CCV_NNC_EXEC_SUCCESS;
	const int vec = (((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 7) == 0) ? 1 : 0;
	hipLaunchKernelGGL(half_down_kernel, dim3(grid_for(vec ? (n + 3) / 4 : n, 256)), dim3(256), 0, stream_of(ctx), in, (half_t*)out, n, vec);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

bool any_half_tensor(ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size)
{
	for (int i = 0; i < input_size; i++)
		if (inputs[i] && CCV_GET_DATA_TYPE(inputs[i]->info.datatype) == CCV_16F) return true;
	for (int i = 0; i < output_size; i++)
		if (outputs[i] && CCV_GET_DATA_TYPE(outputs[i]->info.datatype) == CCV_16F) return true;
	return false;
}

namespace {

// elements from the tensor's first element to one past its last (views: by their strides)
size_t tensor_span(const ccv_nnc_tensor_t* t)
{
	if (!CCV_IS_TENSOR_VIEW(t)) return tensor_count(t->info);
	int st[CCV_NNC_MAX_DIM_ALLOC];
	tensor_strides(t, st);
	const int nd = tensor_nd(t->info.dim);
	if (nd == 0) return 0;
	size_t last = 0;
	for (int i = 0; i < nd; i++) {
		if (t->info.dim[i] <= 0) return 0;
		last += (size_t)(t->info.dim[i] - 1) * (size_t)st[i];
	}
	return last + 1;
}

struct staged_t {
	void* half;   // the tensor's own (half-precision) memory
	size_t span;  // elements
	float* image; // its fp32 image in the arena
	bool is_output, is_input, load;
};

constexpr int MAX_STAGED = 64;

} // namespace

// The reference host's graph runner does not look at what a command returns (lib/nnc/ccv_nnc_graph_run.c calls ccv_nnc_cmd_exec and
// moves on): a refused command would leave its outputs unwritten in silence.  Say so on stderr, a few times per command id.
void warn_refused(const uint32_t cmd, const int ret)
{
	static uint32_t seen[32];
	static int counts[32], nseen = 0;
	if (ret == CCV_NNC_EXEC_SUCCESS) return;
	int i;
	for (i = 0; i < nseen; i++) if (seen[i] == cmd) break;
	if (i == nseen) { if (nseen == 32) return; seen[nseen] = cmd; counts[nseen++] = 0; }
	if (counts[i]++ < 3) fprintf(stderr, "[nnc-mi355x] command 0x%08x refused with %d (INVALID -1 / NO_KERNEL -2 / OOM -3): its outputs were NOT written\n", cmd, ret);
}

// Rows whose kernels read and write their LARGE tensors in half precision themselves (loads / stores of halves, fp32 arithmetic:
// cmd_ew.cpp, cmd_norm.cpp, cmd_pool.cpp, cmd_act_opt.cpp, cmd_bcast.cpp's plane-scale MUL, row_ops.h, group_ops.h, bcast_ops.h, upsample_ops.h, index_ops.h, cmul_ops.h, grad_ops.h).  Bit i of `in` / `out` = that input / output stays in its own memory when every tensor
// named by the masks is a dense CCV_16F tensor; the row's small tensors (batch-norm statistics, ...) still get fp32 images.
static long g_half_staged = 0, g_half_native = 0; // nnc_mi355x_debug_half_counts (test hook; not synchronised: counts, not control)
// NNC_MI355X_HALF_STATS=1: one line per command at unload -- which rows of a run went through fp32 images of their half tensors (and how many tensors)
static struct half_stats_t {
	struct { uint32_t cmd; long calls, tensors; } row[64];
	int n = 0, on = -1;
	~half_stats_t()
	{
		if (on != 1) return;
		for (int i = 0; i < n; i++) fprintf(stderr, "[nnc_mi355x] half tensors staged as fp32 images: %-48s %6ld calls, %6ld tensors\n", command_row_name(row[i].cmd), row[i].calls, row[i].tensors);
	}
} g_half_stats;
static void half_stats_note(const uint32_t cmd, const int tensors)
{
	if (g_half_stats.on < 0) { const char* e = getenv("NNC_MI355X_HALF_STATS"); g_half_stats.on = (e && *e == '1') ? 1 : 0; }
	if (g_half_stats.on != 1 || !tensors) return;
	for (int i = 0; i < g_half_stats.n; i++) if (g_half_stats.row[i].cmd == cmd) { g_half_stats.row[i].calls++; g_half_stats.row[i].tensors += tensors; return; }
	if (g_half_stats.n < 64) { g_half_stats.row[g_half_stats.n].cmd = cmd; g_half_stats.row[g_half_stats.n].calls = 1; g_half_stats.row[g_half_stats.n].tensors = tensors; g_half_stats.n++; }
}
// `when`: null, or the row is native only for the commands it accepts (asked after the masks have matched: every tensor they name is a dense CCV_16F one)
typedef bool (*native_when_f)(const ccv_nnc_cmd_t cmd, int flags, ccv_nnc_tensor_t* const* inputs, int input_size, ccv_nnc_tensor_t* const* outputs, int output_size);
struct native_half_t { uint32_t cmd; unsigned in, out; native_when_f when; };
static bool act_native(const ccv_nnc_cmd_t, int, ccv_nnc_tensor_t* const*, int, ccv_nnc_tensor_t* const*, int) { return tune(TUNE_ACT_HALF_NATIVE) != 0; }
// the backward commands without g (ones) keep their fp32 kernels (cmd_act_opt.cpp)
static bool act_back_native(const ccv_nnc_cmd_t, int, ccv_nnc_tensor_t* const* inputs, int input_size, ccv_nnc_tensor_t* const*, int) { return tune(TUNE_ACT_HALF_NATIVE) != 0 && input_size > 0 && inputs[0]; }
// the optimizers (cmd_act_opt.cpp, optim.h): the amsgrad tensors (input 4, output 3) belong to the state tensors when present
constexpr unsigned OPT_G = 1u << 0, OPT_STATE_IN = (1u << 1) | (1u << 2) | (1u << 3) | (1u << 4), OPT_STATE_OUT = (1u << 0) | (1u << 1) | (1u << 2) | (1u << 3);
static bool opt_native(const ccv_nnc_cmd_t, int, ccv_nnc_tensor_t* const*, int, ccv_nnc_tensor_t* const*, int) { return tune(TUNE_OPT_HALF_NATIVE) != 0; }
static bool none_half(ccv_nnc_tensor_t* const* ts, const int from, const int size) { for (int i = from; i < size; i++) if (ts[i] && CCV_GET_DATA_TYPE(ts[i]->info.datatype) == CCV_16F) return false; return true; }
// g alone: no other tensor is a half one (state tensors of two types keep their fp32 images)
static bool opt_g_native(const ccv_nnc_cmd_t, int, ccv_nnc_tensor_t* const* inputs, int input_size, ccv_nnc_tensor_t* const* outputs, int output_size) { return tune(TUNE_OPT_HALF_NATIVE) != 0 && none_half(inputs, 1, input_size) && none_half(outputs, 0, output_size); }
// the state tensors alone: g is not a half tensor
static bool opt_state_native(const ccv_nnc_cmd_t, int, ccv_nnc_tensor_t* const* inputs, int input_size, ccv_nnc_tensor_t* const*, int) { return tune(TUNE_OPT_HALF_NATIVE) != 0 && none_half(inputs, 0, input_size < 1 ? input_size : 1); }
// row_ops.h: LAYER_NORM (affine and not: the statistics sit in other slots), RMSNORM, SOFTMAX.  The predicates are cmd_rownorm.cpp's / cmd_act_opt.cpp's
static bool lnorm_affine_native(const ccv_nnc_cmd_t cmd, int flags, ccv_nnc_tensor_t* const* inputs, int input_size, ccv_nnc_tensor_t* const* outputs, int output_size) { return cmd.info.lnorm.elementwise_affine && rownorm_half_applies(cmd, flags, inputs, input_size, outputs, output_size); }
static bool lnorm_plain_native(const ccv_nnc_cmd_t cmd, int flags, ccv_nnc_tensor_t* const* inputs, int input_size, ccv_nnc_tensor_t* const* outputs, int output_size) { return !cmd.info.lnorm.elementwise_affine && rownorm_half_applies(cmd, flags, inputs, input_size, outputs, output_size); }
// group_ops.h: GROUP_NORM, the slots of LAYER_NORM.  The predicate is cmd_groupnorm.cpp's
static bool gnorm_affine_native(const ccv_nnc_cmd_t cmd, int flags, ccv_nnc_tensor_t* const* inputs, int input_size, ccv_nnc_tensor_t* const* outputs, int output_size) { return cmd.info.gnorm.elementwise_affine && gnorm_half_applies(cmd, flags, inputs, input_size, outputs, output_size); }
static bool gnorm_plain_native(const ccv_nnc_cmd_t cmd, int flags, ccv_nnc_tensor_t* const* inputs, int input_size, ccv_nnc_tensor_t* const* outputs, int output_size) { return !cmd.info.gnorm.elementwise_affine && gnorm_half_applies(cmd, flags, inputs, input_size, outputs, output_size); }
static const native_half_t g_native_half[] = {
	{ CCV_NNC_RELU_FORWARD, 1u << 0, 1u << 0 },
	{ CCV_NNC_RELU_BACKWARD, (1u << 0) | (1u << 2), 1u << 0 },            // g, (a unused), b -> h
	{ CCV_NNC_EWSUM_FORWARD, ~0u, 1u << 0 },
	{ CCV_NNC_EWSUM_BACKWARD, 1u << 0, ~0u },
	{ CCV_NNC_BATCH_NORM_FORWARD, 1u << 0, 1u << 0 },                     // x -> y
	{ CCV_NNC_BATCH_NORM_BACKWARD, (1u << 0) | (1u << 5), 1u << 0 },      // g, x -> h
	{ CCV_NNC_MAX_POOL_FORWARD, 1u << 0, 1u << 0 },
	{ CCV_NNC_MAX_POOL_BACKWARD, (1u << 0) | (1u << 1) | (1u << 2), 1u << 0 }, // g, x, y -> h
	{ CCV_NNC_AVERAGE_POOL_FORWARD, 1u << 0, 1u << 0 },
	{ CCV_NNC_AVERAGE_POOL_BACKWARD, 1u << 0, 1u << 0 },
	{ CCV_NNC_SGD_FORWARD, (1u << 0) | (1u << 1) | (1u << 2), (1u << 0) | (1u << 1) }, // g, a, m -> b, n
	{ CCV_NNC_SOFTMAX_CROSSENTROPY_FORWARD, 1u << 0, 1u << 1 },           // logits -> softmax (labels and the loss: fp32 images, a value per row)
	{ CCV_NNC_SOFTMAX_CROSSENTROPY_BACKWARD, 1u << 5, 1u << 0 },          // softmax -> h
	// cmd_act_opt.cpp: a -> b;  g, (a unused), b -> h  or  g, a -> h
	{ CCV_NNC_SIGMOID_FORWARD, 1u << 0, 1u << 0, act_native },
	{ CCV_NNC_SIGMOID_BACKWARD, (1u << 0) | (1u << 2), 1u << 0, act_back_native },
	{ CCV_NNC_TANH_FORWARD, 1u << 0, 1u << 0, act_native },
	{ CCV_NNC_TANH_BACKWARD, (1u << 0) | (1u << 2), 1u << 0, act_back_native },
	{ CCV_NNC_GELU_FORWARD, 1u << 0, 1u << 0, act_native },
	{ CCV_NNC_GELU_BACKWARD, (1u << 0) | (1u << 1), 1u << 0, act_back_native },
	{ CCV_NNC_SWISH_FORWARD, 1u << 0, 1u << 0, act_native },
	{ CCV_NNC_SWISH_BACKWARD, (1u << 0) | (1u << 1), 1u << 0, act_back_native },
	{ CCV_NNC_LEAKY_RELU_FORWARD, 1u << 0, 1u << 0, act_native },
	{ CCV_NNC_LEAKY_RELU_BACKWARD, (1u << 0) | (1u << 2), 1u << 0, act_back_native },
	{ CCV_NNC_DROPOUT_FORWARD, 1u << 0, 1u << 0, act_native },            // a -> b (the mask is opaque, below)
	{ CCV_NNC_DROPOUT_BACKWARD, 1u << 0, 1u << 0, act_native },           // g -> h
	// cmd_bcast.cpp: only the squeeze-excite pattern of mul_planes.h; every other MUL runs on fp32 images
	{ CCV_NNC_MUL_FORWARD, (1u << 0) | (1u << 1), 1u << 0, mul_planes_applies },            // a, b -> c
	{ CCV_NNC_MUL_BACKWARD, (1u << 0) | (1u << 1) | (1u << 2), (1u << 0) | (1u << 1), mul_planes_applies }, // g, a, b -> da, db
	// bcast_ops.h: ADD, same-shape MUL (behind the plane-scale rows), REDUCE_SUM / REDUCE_MEAN and SCALAR_MUL where bcast_half_plan takes the shapes (flat, a period, runs)
	{ CCV_NNC_MUL_FORWARD, (1u << 0) | (1u << 1), 1u << 0, bcast_half_applies },
	{ CCV_NNC_MUL_BACKWARD, (1u << 0) | (1u << 1) | (1u << 2), (1u << 0) | (1u << 1), bcast_half_applies },
	// grad_ops.h (behind the MUL rows above: whatever those take they still take): a dense half tensor by a one-element tensor -- both operands half; the large
	// one first, then second, with a CCV_32F scalar, which is no half and passes as itself
	{ CCV_NNC_MUL_FORWARD, (1u << 0) | (1u << 1), 1u << 0, grad_half_applies },
	{ CCV_NNC_MUL_FORWARD, 1u << 0, 1u << 0, grad_half_applies },
	{ CCV_NNC_MUL_FORWARD, 1u << 1, 1u << 0, grad_half_applies },
	{ CCV_NNC_ADD_FORWARD, (1u << 0) | (1u << 1), 1u << 0, bcast_half_applies },             // a, b -> c
	{ CCV_NNC_ADD_BACKWARD, 1u << 0, (1u << 0) | (1u << 1), bcast_half_applies },            // g -> da, db
	{ CCV_NNC_REDUCE_SUM_FORWARD, 1u << 0, 1u << 0, bcast_half_applies },                    // a -> b
	{ CCV_NNC_REDUCE_SUM_BACKWARD, 1u << 0, 1u << 0, bcast_half_applies },                   // g -> h
	{ CCV_NNC_REDUCE_MEAN_FORWARD, 1u << 0, 1u << 0, bcast_half_applies },
	{ CCV_NNC_REDUCE_MEAN_BACKWARD, 1u << 0, 1u << 0, bcast_half_applies },
	{ CCV_NNC_SCALAR_MUL_FORWARD, 1u << 0, 1u << 0, bcast_half_applies },                    // a -> b (cmd_ew.cpp)
	{ CCV_NNC_SCALAR_MUL_BACKWARD, 1u << 0, 1u << 0, bcast_half_applies },                   // g -> h
	// optim.h: g, a, m, v[, vm] -> b, n, u[, um].  Three rows per command, tried in order: every tensor half; g alone (half gradients into fp32 master
	// parameters); the parameter and state tensors alone (fp32 gradients)
#define OPT_ROWS(CMD) { CMD, OPT_G | OPT_STATE_IN, OPT_STATE_OUT, opt_native }, { CMD, OPT_G, 0, opt_g_native }, { CMD, OPT_STATE_IN, OPT_STATE_OUT, opt_state_native }
	OPT_ROWS(CCV_NNC_RMSPROP_FORWARD),
	OPT_ROWS(CCV_NNC_ADAM_FORWARD),
	OPT_ROWS(CCV_NNC_ADAMW_FORWARD),
	OPT_ROWS(CCV_NNC_LAMB_FORWARD),
#undef OPT_ROWS
	// row_ops.h.  Two rows per command (and per layer-norm variant), tried in order: every USED tensor half ("hh": what an all-half graph issues -- the parameters
	// and statistics take the input's type); the maps alone ("hf": a half parameter or statistic gets its small fp32 image).  Unused slots are not named.
	{ CCV_NNC_LAYER_NORM_FORWARD, (1u << 0) | (1u << 1) | (1u << 2), (1u << 0) | (1u << 1) | (1u << 2), lnorm_affine_native }, // a, scale, bias -> b, saved_mean, saved_inv_std
	{ CCV_NNC_LAYER_NORM_FORWARD, 1u << 0, (1u << 0) | (1u << 1) | (1u << 2), lnorm_plain_native },                            // a -> b, saved_mean, saved_inv_std
	{ CCV_NNC_LAYER_NORM_FORWARD, 1u << 0, 1u << 0, rownorm_half_applies },
	{ CCV_NNC_LAYER_NORM_BACKWARD, (1u << 0) | (1u << 3) | (1u << 4) | (1u << 7) | (1u << 8), (1u << 0) | (1u << 1) | (1u << 2), lnorm_affine_native }, // g, a, scale, saved_mean, saved_inv_std -> h, dscale, dbias
	{ CCV_NNC_LAYER_NORM_BACKWARD, (1u << 0) | (1u << 3) | (1u << 5) | (1u << 6), (1u << 0) | (1u << 1) | (1u << 2), lnorm_plain_native },             // g, a, saved_mean, saved_inv_std -> h
	{ CCV_NNC_LAYER_NORM_BACKWARD, (1u << 0) | (1u << 3), 1u << 0, rownorm_half_applies },
	// group_ops.h: the same two rows per variant
	{ CCV_NNC_GROUP_NORM_FORWARD, (1u << 0) | (1u << 1) | (1u << 2), (1u << 0) | (1u << 1) | (1u << 2), gnorm_affine_native }, // a, scale, bias -> b, saved_mean, saved_inv_std
	{ CCV_NNC_GROUP_NORM_FORWARD, 1u << 0, (1u << 0) | (1u << 1) | (1u << 2), gnorm_plain_native },                            // a -> b, saved_mean, saved_inv_std
	{ CCV_NNC_GROUP_NORM_FORWARD, 1u << 0, 1u << 0, gnorm_half_applies },
	{ CCV_NNC_GROUP_NORM_BACKWARD, (1u << 0) | (1u << 3) | (1u << 4) | (1u << 7) | (1u << 8), (1u << 0) | (1u << 1) | (1u << 2), gnorm_affine_native }, // g, a, scale, saved_mean, saved_inv_std -> h, dscale, dbias
	{ CCV_NNC_GROUP_NORM_BACKWARD, (1u << 0) | (1u << 3) | (1u << 5) | (1u << 6), (1u << 0) | (1u << 1) | (1u << 2), gnorm_plain_native },             // g, a, saved_mean, saved_inv_std -> h
	{ CCV_NNC_GROUP_NORM_BACKWARD, (1u << 0) | (1u << 3), 1u << 0, gnorm_half_applies },
	{ CCV_NNC_RMSNORM_FORWARD, (1u << 0) | (1u << 1), (1u << 0) | (1u << 1), rownorm_half_applies },                           // a, scale -> b, saved_inv_std
	{ CCV_NNC_RMSNORM_FORWARD, 1u << 0, 1u << 0, rownorm_half_applies },
	{ CCV_NNC_RMSNORM_BACKWARD, (1u << 0) | (1u << 2) | (1u << 3) | (1u << 5), (1u << 0) | (1u << 1), rownorm_half_applies },  // g, a, scale, saved_inv_std -> h, dscale
	{ CCV_NNC_RMSNORM_BACKWARD, (1u << 0) | (1u << 2), 1u << 0, rownorm_half_applies },
	{ CCV_NNC_SOFTMAX_FORWARD, 1u << 0, 1u << 0, softmax_half_applies },                                                       // a -> b
	{ CCV_NNC_SOFTMAX_BACKWARD, (1u << 0) | (1u << 2), 1u << 0, softmax_half_applies },                                        // g, (a unused), b -> h
	// upsample_ops.h: nearest and bilinear, NCHW and NHWC, where upsample_half_plan takes the geometry
	{ CCV_NNC_UPSAMPLE_FORWARD, 1u << 0, 1u << 0, upsample_half_applies },                                                     // a -> b
	{ CCV_NNC_UPSAMPLE_BACKWARD, 1u << 0, 1u << 0, upsample_half_applies },                                                    // g -> h
	// index_ops.h: gather, ordered scatter-add and pad, where index_half_plan / pad_half_plan take the command.  The indices are never named (they are no halves)
	{ CCV_NNC_INDEX_SELECT_FORWARD, 1u << 0, 1u << 0, index_pad_half_applies },                                                // a, (indices) -> b
	{ CCV_NNC_INDEX_SELECT_BACKWARD, 1u << 0, 1u << 0, index_pad_half_applies },                                               // g, _, (indices) -> h
	{ CCV_NNC_PAD_FORWARD, 1u << 0, 1u << 0, index_pad_half_applies },                                                         // a -> b
	{ CCV_NNC_PAD_BACKWARD, 1u << 0, 1u << 0, index_pad_half_applies },                                                        // g -> h
	// cmul_ops.h: the complex multiply (rotary embeddings), where cmul_half_plan takes every requested output
	{ CCV_NNC_CMUL_FORWARD, (1u << 0) | (1u << 1), 1u << 0, cmul_half_applies },                                               // a, b -> c
	{ CCV_NNC_CMUL_BACKWARD, (1u << 0) | (1u << 1) | (1u << 2), (1u << 0) | (1u << 1), cmul_half_applies },                    // g, a, b -> da, db
	// grad_ops.h: a whole dense half tensor reduced to one element, where grad_half_plan takes the command.  A half result is named first: the row without it
	// would stage it.  CCV_32F / CCV_32S results are no halves and pass as themselves
	{ CCV_NNC_REDUCE_NORM2_FORWARD, 1u << 0, 1u << 0, grad_half_applies },                                                     // a -> b, both half
	{ CCV_NNC_REDUCE_NORM2_FORWARD, 1u << 0, 0, grad_half_applies },                                                           // a -> b (fp32)
	{ CCV_NNC_REDUCE_ISNAN_FORWARD, 1u << 0, 0, grad_half_applies },                                                           // a -> b (int32)
};
static const native_half_t* native_half_row(const ccv_nnc_cmd_t command, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size)
{
	if (flags & CCV_NNC_ACCUMULATE_OUTPUT) return 0;
	const uint32_t cmd = command.cmd;
	for (const native_half_t& r : g_native_half) {
		if (r.cmd != cmd) continue;
		int seen = 0;
		bool fits = true;
		for (int i = 0; fits && i < input_size && i < 32; i++)
			if (((r.in >> i) & 1) && inputs[i]) { fits = CCV_GET_DATA_TYPE(inputs[i]->info.datatype) == CCV_16F && !CCV_IS_TENSOR_VIEW(inputs[i]); seen++; }
		for (int i = 0; fits && i < output_size && i < 32; i++)
			if (((r.out >> i) & 1) && outputs[i]) { fits = CCV_GET_DATA_TYPE(outputs[i]->info.datatype) == CCV_16F && !CCV_IS_TENSOR_VIEW(outputs[i]); seen++; }
		if (fits && seen && (!r.when || r.when(command, flags, inputs, input_size, outputs, output_size))) return &r;
		// (a command may have several rows -- the optimizers' type combinations: the next one of the same command is tried)
	}
	return 0;
}

int half_staged_exec(const nnc_exec_user_f inner, void* const user, const ccv_nnc_cmd_t cmd, const ccv_nnc_hint_t hint, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, ccv_nnc_stream_context_t* const ctx)
{
	MarkerScope marker(cmd.cmd); // every row registered through NNC_HALF_STAGED passes here: the per-command roctx range
	if (!any_half_tensor(inputs, input_size, outputs, output_size)) {
		const int r = inner(user, cmd, hint, flags, inputs, input_size, outputs, output_size, ctx);
		warn_refused(cmd.cmd, r);
		return r;
	}
	if (input_size + output_size > MAX_STAGED) return CCV_NNC_EXEC_INVALID;
	staged_t st[MAX_STAGED];
	int nst = 0;
	// shadow tensor structs: a view keeps its stride block, so the larger struct is copied for every tensor
	ccv_nnc_tensor_view_t shadow[MAX_STAGED];
	ccv_nnc_tensor_t* in_s[MAX_STAGED];
	ccv_nnc_tensor_t* out_s[MAX_STAGED];
	int which[MAX_STAGED]; // staged entry of shadow i, -1 = the tensor itself is passed on
	size_t total = 0;
	auto visit = [&](ccv_nnc_tensor_t* t, const bool is_output, const int slot) {
		which[slot] = -1;
		if (!t || CCV_GET_DATA_TYPE(t->info.datatype) != CCV_16F) return;
		const size_t span = tensor_span(t);
		int e = -1;
		for (int i = 0; i < nst; i++)
			if (st[i].half == (void*)t->data.u8) { e = i; break; } // the same memory through two tensor structs (in-place commands): one image
		if (e < 0) {
			e = nst++;
			st[e].half = t->data.u8; st[e].span = span; st[e].image = 0; st[e].is_output = st[e].is_input = st[e].load = false;
		} else if (span > st[e].span) st[e].span = span;
		if (is_output) {
			st[e].is_output = true;
			// the old value under accumulation must be in the image (a view's gaps need not: they are never written back)
			if (flags & CCV_NNC_ACCUMULATE_OUTPUT) st[e].load = true;
		} else { st[e].is_input = true; st[e].load = true; }
		which[slot] = e;
	};
	// opaque tensors keep their own memory: the dropout mask is a byte buffer the host merely SIZES through a tensor of the data's
	// type (ccv_nnc_dropout.c:21-45) -- output 1 of the forward command, input 4 of the backward one
	// The LSTM's reserved space likewise (output 3 forward, input 12 backward): ccv_nnc_lstm.c:55-61 sizes it as `bytes` ELEMENTS of the data's type, so a CCV_16F
	// one spans at least the bytes fp32 planes need and the kernels keep their tape (gates, tanh(c), cell states, dropout scales) in fp32 inside it -- nothing is
	// rounded to half between the forward and the backward command, no cell state can overflow the half range, and the space is not converted twice per call
	const int opaque_in = cmd.cmd == CCV_NNC_DROPOUT_BACKWARD ? 4 : (cmd.cmd == CCV_NNC_LSTM_BACKWARD ? 12 : -1), opaque_out = cmd.cmd == CCV_NNC_DROPOUT_FORWARD ? 1 : (cmd.cmd == CCV_NNC_LSTM_FORWARD ? 3 : -1);
	const native_half_t* const native = native_half_row(cmd, flags, inputs, input_size, outputs, output_size);
	for (int i = 0; i < input_size; i++) { if (i == opaque_in || (native && i < 32 && ((native->in >> i) & 1))) which[i] = -1; else visit(inputs[i], false, i); }
	for (int i = 0; i < output_size; i++) { if (i == opaque_out || (native && i < 32 && ((native->out >> i) & 1))) which[input_size + i] = -1; else visit(outputs[i], true, input_size + i); }
	for (int i = 0; i < nst; i++) total += (st[i].span * sizeof(float) + 255) & ~(size_t)255;
	g_half_staged += nst;
	half_stats_note(cmd.cmd, nst);
	if (native)
		for (int i = 0; i < input_size + output_size; i++) {
			ccv_nnc_tensor_t* const t = i < input_size ? inputs[i] : outputs[i - input_size];
			const int k = i < input_size ? i : i - input_size;
			if (t && k < 32 && (((i < input_size ? native->in : native->out) >> k) & 1)) g_half_native++;
		}
	char* arena = (char*)nnc_staging_of(ctx, total);
	if (total && !arena) return CCV_NNC_EXEC_OOM;
	size_t off = 0;
	for (int i = 0; i < nst; i++) {
		st[i].image = (float*)(arena + off);
		off += (st[i].span * sizeof(float) + 255) & ~(size_t)255;
		if (st[i].load) half_to_float(st[i].half, st[i].image, st[i].span, ctx);
	}
	auto make_shadow = [&](ccv_nnc_tensor_t* t, const int slot) -> ccv_nnc_tensor_t* {
		if (!t || which[slot] < 0) return t;
		if (CCV_IS_TENSOR_VIEW(t)) memcpy(&shadow[slot], t, sizeof(ccv_nnc_tensor_view_t));
		else { memset(&shadow[slot], 0, sizeof(ccv_nnc_tensor_view_t)); memcpy(&shadow[slot], t, sizeof(ccv_nnc_tensor_t)); }
		ccv_nnc_tensor_t* s = (ccv_nnc_tensor_t*)&shadow[slot];
		s->info.datatype = CCV_32F;
		s->data.f32 = st[which[slot]].image;
		s->dataof = 0;
		s->data_size = 0;
		s->alias_ref = 0;
		return s;
	};
	for (int i = 0; i < input_size; i++) in_s[i] = make_shadow(inputs[i], i);
	for (int i = 0; i < output_size; i++) out_s[i] = make_shadow(outputs[i], input_size + i);
	// With staged tensors `inner` must run on the spot: its shadow tensors point into the arena and its outputs are converted back right below.  The look-ahead
	// (peephole.cpp) would record a batch norm / convolution here; a recorded command launched by a flush has no caller to report a failure to, and this
	// function went on to convert the never-written image down to half and return SUCCESS.  So: no recording underneath.
	if (nst) deferred_suppress(1);
	const int ret = inner(user, cmd, hint, flags, in_s, input_size, out_s, output_size, ctx);
	if (nst) deferred_suppress(-1);
	warn_refused(cmd.cmd, ret);
	if (ret != CCV_NNC_EXEC_SUCCESS) return ret;
	// per OUTPUT tensor, not per image: two views of one parent share an image and each writes its own elements
	for (int i = 0; i < output_size; i++) {
		const int e = which[input_size + i];
		if (e < 0 || !outputs[i]) continue;
		bool done = false;
		for (int j = 0; j < i && !done; j++) done = which[input_size + j] == e && outputs[j] && outputs[j]->data.u8 == outputs[i]->data.u8 && !CCV_IS_TENSOR_VIEW(outputs[j]) && !CCV_IS_TENSOR_VIEW(outputs[i]);
		if (done) continue;
		if (CCV_IS_TENSOR_VIEW(outputs[i]) && !tensor_contiguous(outputs[i])) float_to_half_view(st[e].image, st[e].half, outputs[i], ctx);
		else float_to_half(st[e].image, st[e].half, tensor_count(outputs[i]->info), ctx);
	}
	return CCV_NNC_EXEC_SUCCESS;
}
int half_staged_exec(const nnc_exec_f inner, const ccv_nnc_cmd_t cmd, const ccv_nnc_hint_t hint, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, ccv_nnc_stream_context_t* const ctx)
{
	return half_staged_exec([](void* const f, const ccv_nnc_cmd_t cmd, const ccv_nnc_hint_t hint, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, ccv_nnc_stream_context_t* const ctx) { return ((nnc_exec_f)f)(cmd, hint, flags, inputs, input_size, outputs, output_size, ctx); }, (void*)inner, cmd, hint, flags, inputs, input_size, outputs, output_size, ctx);
}

} // namespace nnc

extern "C" void nnc_mi355x_debug_half_counts(long* staged, long* native)
{
	if (staged) *staged = nnc::g_half_staged;
	if (native) *native = nnc::g_half_native;
}
