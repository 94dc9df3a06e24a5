// Activations, plain softmax and the Adam / AdamW / RMSProp / LAMB update on gfx950 -- the element-wise rows the reference's other
// trainers need beside SGD.  All HBM-bound: 16 bytes per lane when aligned; the activations grid-stride, the optimizers (optim.h) a tile per workgroup.  The five activation families run
// CCV_16F tensors as halves themselves (act_map_kernel; half_stage.cpp g_native_half, tunable ACT_HALF_NATIVE).
// Oracle semantics (CPU reference, fp32 storage, arithmetic promoted to double there; float here, within 1e-6):
//   sigmoid     lib/nnc/cmd/sigmoid/ccv_nnc_sigmoid_cpu_ref.c:13-66        b = 1/(1+e^-a);  h = g b (1-b)      (g may be absent: ones)
//   tanh        lib/nnc/cmd/tanh/ccv_nnc_tanh_cpu_ref.c:13-62              b = tanh a;      h = g (1-b^2)
//   gelu        lib/nnc/cmd/gelu/ccv_nnc_gelu_cpu_ref.c:13-91              erf form and the tanh approximation (cmd.info.gelu.tanh)
//   swish       lib/nnc/cmd/swish/ccv_nnc_swish_cpu_ref.c:13-79            b = a/(1+e^-a);  h = g (a (y - y^2) + y), y = sigmoid a
//   leaky relu  lib/nnc/cmd/leaky_relu/ccv_nnc_leaky_relu_cpu_ref.c:13-60  b = a >= 0 ? a : s a;  h = b >= 0 ? g : s g
//   softmax     lib/nnc/cmd/softmax/ccv_nnc_softmax_cpu_ref.c:13-73        rows = dim[0] (1-d: one row); h = (g - sum(g b)) b
//   adam        lib/nnc/cmd/adam/ccv_nnc_adam_cpu_ref.c:16-175             inputs (g, a, m, v[, vm]) -> (b, n, u[, um]); L2 decay inside the gradient
//   adamw       lib/nnc/cmd/adam/ccv_nnc_adamw_cpu_ref.c:16-174            decoupled decay: b = a - rate decay a - ...
//   rmsprop     lib/nnc/cmd/rmsprop/ccv_nnc_rmsprop_cpu_ref.c:16-108       inputs (g, a, m, v) -> (b, n, u)
//   lamb        lib/nnc/cmd/lamb/ccv_nnc_lamb_cpu_ref.c:16-140             Adam-style update scaled per TENSOR by |w| / |update| (norms in double)
#include "common.h"
#include "optim.h"
#include "row_ops.h"

using namespace nnc;

namespace {

constexpr int EW_THREADS = 256;

// out[i] = f(x[i], y[i]) over contiguous tensors of one element type; NIN = how many inputs are read.  T = float, or _Float16 for the CCV_16F tensors of the
// half-precision trainers: loaded and stored as halves (a lane takes 16 bytes: 4 floats / 8 halves), the functors below compute in fp32 as they always did and the
// result is rounded once, to nearest even, by the store.  nv = whole 16-byte vectors (0 when a base is not 16-byte aligned: every element takes the scalar loop).
typedef _Float16 half_t;
template <class T> struct pack16 { typedef T type __attribute__((ext_vector_type(16 / sizeof(T)))); };
template <class F, int NIN, class T>
__global__ void __launch_bounds__(EW_THREADS) act_map_kernel(F f, T* out, const T* in0, const T* in1, const size_t nv, const size_t n)
{
	constexpr int W = 16 / sizeof(T);
	typedef typename pack16<T>::type V;
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	for (size_t i = tid; i < nv; i += stride) {
		const V a = ((const V*)in0)[i];
		V b = a;
		if (NIN > 1) b = ((const V*)in1)[i];
		V r;
#pragma unroll
		for (int e = 0; e < W; e++) r[e] = (T)f32_rounded(f((float)a[e], NIN > 1 ? (float)b[e] : 0.f));
		((V*)out)[i] = r;
	}
	for (size_t i = nv * W + tid; i < n; i += stride) out[i] = (T)f32_rounded(f((float)in0[i], NIN > 1 ? (float)in1[i] : 0.f));
}

template <class F, int NIN, class T>
static int act_map(F f, T* out, const T* in0, const T* in1, const size_t n, ccv_nnc_stream_context_t* ctx)
{
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	constexpr int W = 16 / sizeof(T);
	const bool vec = aligned16(out) && aligned16(in0) && (NIN < 2 || aligned16(in1));
	const size_t nv = vec ? n / W : 0;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(act_map_kernel<F, NIN, T>), dim3(grid_for(vec ? nv + (W - 1) : n, EW_THREADS)), dim3(EW_THREADS), 0, stream_of(ctx), f, out, in0, in1, nv, n);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}
// the tensors' own element type: every tensor handed over is of one type (half_stage.cpp keeps the tensors of these rows in half precision only when all of them are)
template <class F, int NIN>
static int act_map_any(F f, const int datatype, ccv_nnc_tensor_t* out, const ccv_nnc_tensor_t* in0, const ccv_nnc_tensor_t* in1, const size_t n, ccv_nnc_stream_context_t* ctx)
{
	if (CCV_GET_DATA_TYPE(datatype) == CCV_16F) return act_map<F, NIN, half_t>(f, (half_t*)out->data.u8, (const half_t*)in0->data.u8, in1 ? (const half_t*)in1->data.u8 : 0, n, ctx);
	return act_map<F, NIN, float>(f, out->data.f32, (const float*)in0->data.f32, in1 ? (const float*)in1->data.f32 : 0, n, ctx);
}

__device__ __forceinline__ float sigmoidf_(const float x) { return 1.f / (1.f + expf(-x)); }

struct OpSigmoid { __device__ float operator()(float a, float) const { return sigmoidf_(a); } };
struct OpSigmoidBack { __device__ float operator()(float b, float g) const { return g * b * (1.f - b); } };      // (b, g)
struct OpSigmoidBackOnes { __device__ float operator()(float b, float) const { return b * (1.f - b); } };
struct OpTanh { __device__ float operator()(float a, float) const { return tanhf(a); } };
struct OpTanhBack { __device__ float operator()(float b, float g) const { return g * (1.f - b * b); } };
struct OpTanhBackOnes { __device__ float operator()(float b, float) const { return 1.f - b * b; } };
struct OpGeluErf { __device__ float operator()(float x, float) const { return x * 0.5f * (1.f + erff(x * 0.70710678118654752440f)); } };
struct OpGeluTanh { __device__ float operator()(float x, float) const { return 0.5f * x * (1.f + tanhf(0.797884560802865355f * (x + 0.044715f * x * x * x))); } };
struct OpGeluErfBack { // (x, g)
	__device__ float operator()(float x, float g) const
	{
		const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752440f));
		const float pdf = expf(-0.5f * x * x) * 0.797884560802865355f;
		return g * (cdf + x * pdf);
	}
};
struct OpGeluTanhBack {
	__device__ float operator()(float x, float g) const
	{
		const float x_sq = x * x;
		const float t = tanhf(0.797884560802865355f * (x + 0.044715f * x_sq * x));
		const float left_d = 0.5f * (1.f + t);
		const float right_d = 0.5f * x * (1.f - t * t) * 0.797884560802865355f * (1.f + 3.f * 0.044715f * x_sq);
		return g * (left_d + right_d);
	}
};
struct OpSwish { __device__ float operator()(float a, float) const { return a * sigmoidf_(a); } };
struct OpSwishBack { __device__ float operator()(float x, float g) const { const float y = sigmoidf_(x); return g * (x * (y - y * y) + y); } };
struct OpLeaky { float s; __device__ float operator()(float a, float) const { return a >= 0.f ? a : a * s; } };
struct OpLeakyBack { float s; __device__ float operator()(float b, float g) const { return b >= 0.f ? g : s * g; } }; // (b, g)

static bool same_count(const ccv_nnc_tensor_t* a, const ccv_nnc_tensor_t* b) { return tensor_count(a->info) == tensor_count(b->info); }
static bool dense_f32(const ccv_nnc_tensor_t* t) { return t && tensor_contiguous(t) && CCV_GET_DATA_TYPE(t->info.datatype) == CCV_32F; }
// dense, and of datatype dt
static bool dense_of(const ccv_nnc_tensor_t* t, const int dt) { return t && tensor_contiguous(t) && CCV_GET_DATA_TYPE(t->info.datatype) == dt; }
// CCV_32F or CCV_16F (the latter only ever arrives through a native row of half_stage.cpp's table), else 0
static int float_type(const ccv_nnc_tensor_t* t)
{
	const int dt = t ? CCV_GET_DATA_TYPE(t->info.datatype) : 0;
	return dt == CCV_32F || dt == CCV_16F ? dt : 0;
}

// forward: inputs[0] = a -> outputs[0] = b
template <class F>
static int unary_forw(F f, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, ccv_nnc_stream_context_t* const ctx)
{
	if (input_size < 1 || output_size < 1) return CCV_NNC_EXEC_INVALID;
	const int dt = float_type(inputs[0]);
	if (!dt || !dense_of(inputs[0], dt) || !dense_of(outputs[0], dt) || !same_count(inputs[0], outputs[0])) return CCV_NNC_EXEC_INVALID;
	return act_map_any<F, 1>(f, dt, outputs[0], inputs[0], 0, tensor_count(inputs[0]->info), ctx);
}
// backward from the forward OUTPUT: inputs (g [may be null], _, b) -> h
template <class F, class FONES>
static int back_from_output(F f, FONES fones, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, ccv_nnc_stream_context_t* const ctx)
{
	if (input_size < 3 || output_size < 1) return CCV_NNC_EXEC_INVALID;
	const int dt = float_type(inputs[2]);
	if (!dt || !dense_of(inputs[2], dt) || !dense_of(outputs[0], dt) || !same_count(inputs[2], outputs[0])) return CCV_NNC_EXEC_INVALID;
	const ccv_nnc_tensor_t* g = inputs[0];
	const size_t n = tensor_count(inputs[2]->info);
	if (!g) return dt == CCV_32F ? act_map<FONES, 1, float>(fones, outputs[0]->data.f32, (const float*)inputs[2]->data.f32, 0, n, ctx) : CCV_NNC_EXEC_INVALID; // (halves without g: fp32 images, half_stage.cpp)
	if (!dense_of(g, dt) || !same_count(g, outputs[0])) return CCV_NNC_EXEC_INVALID;
	return act_map_any<F, 2>(f, dt, outputs[0], inputs[2], g, n, ctx);
}
// backward from the forward INPUT: inputs (g, a) -> h
template <class F>
static int back_from_input(F f, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, ccv_nnc_stream_context_t* const ctx)
{
	if (input_size < 2 || output_size < 1) return CCV_NNC_EXEC_INVALID;
	const int dt = float_type(inputs[0]);
	if (!dt || !dense_of(inputs[0], dt) || !dense_of(inputs[1], dt) || !dense_of(outputs[0], dt) || !same_count(inputs[0], inputs[1]) || !same_count(inputs[0], outputs[0])) return CCV_NNC_EXEC_INVALID;
	return act_map_any<F, 2>(f, dt, outputs[0], inputs[1], inputs[0], tensor_count(inputs[0]->info), ctx);
}

#define EXEC_ARGS const ccv_nnc_cmd_t cmd, const ccv_nnc_hint_t hint, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, ccv_nnc_stream_context_t* const stream_context
#define IO inputs, input_size, outputs, output_size, stream_context

static int _sigmoid_forw(EXEC_ARGS) { return unary_forw(OpSigmoid(), IO); }
static int _sigmoid_back(EXEC_ARGS) { return back_from_output(OpSigmoidBack(), OpSigmoidBackOnes(), IO); }
static int _tanh_forw(EXEC_ARGS) { return unary_forw(OpTanh(), IO); }
static int _tanh_back(EXEC_ARGS) { return back_from_output(OpTanhBack(), OpTanhBackOnes(), IO); }
static int _gelu_forw(EXEC_ARGS) { return cmd.info.gelu.tanh ? unary_forw(OpGeluTanh(), IO) : unary_forw(OpGeluErf(), IO); }
static int _gelu_back(EXEC_ARGS) { return cmd.info.gelu.tanh ? back_from_input(OpGeluTanhBack(), IO) : back_from_input(OpGeluErfBack(), IO); }
static int _swish_forw(EXEC_ARGS) { return unary_forw(OpSwish(), IO); }
static int _swish_back(EXEC_ARGS) { return back_from_input(OpSwishBack(), IO); }
static int _leaky_forw(EXEC_ARGS) { OpLeaky f = { cmd.info.leaky_relu.negative_slope }; return unary_forw(f, IO); }
static int _leaky_back(EXEC_ARGS)
{ // (g, _, b) -> h, g required (leaky_relu_cpu_ref.c:38-60)
	if (input_size < 3 || !inputs[0]) return CCV_NNC_EXEC_INVALID;
	OpLeakyBack f = { cmd.info.leaky_relu.negative_slope };
	return back_from_output(f, f, IO);
}

// ---- softmax over rows: one 256-thread block per row, two-pass (max, sum of exp) with the row kept in registers/L2 ---------
__device__ __forceinline__ float block_reduce(float v, float* red, const bool is_max)
{
	for (int o = 32; o > 0; o >>= 1) { const float w = __shfl_xor(v, o); v = is_max ? fmaxf(v, w) : v + w; }
	const int wave = threadIdx.x >> 6;
	__syncthreads();
	if ((threadIdx.x & 63) == 0) red[wave] = v;
	__syncthreads();
	float r = red[0];
	for (int i = 1; i < 4; i++) r = is_max ? fmaxf(r, red[i]) : r + red[i];
	return r;
}
__global__ void __launch_bounds__(256) softmax_forw_kernel(const float* a, float* b, const int count)
{
	__shared__ float red[4];
	const float* const ap = a + (size_t)blockIdx.x * count;
	float* const bp = b + (size_t)blockIdx.x * count;
	float m = -INFINITY;
	for (int j = threadIdx.x; j < count; j += 256) m = fmaxf(m, ap[j]);
	m = block_reduce(m, red, true);
	float s = 0.f;
	for (int j = threadIdx.x; j < count; j += 256) { const float e = expf(ap[j] - m); bp[j] = e; s += e; }
	s = block_reduce(s, red, false);
	const float inv = 1.f / s;
	for (int j = threadIdx.x; j < count; j += 256) bp[j] *= inv;
}
__global__ void __launch_bounds__(256) softmax_back_kernel(const float* g, const float* b, float* h, const int count)
{
	__shared__ float red[4];
	const size_t o = (size_t)blockIdx.x * count;
	float s = 0.f;
	for (int j = threadIdx.x; j < count; j += 256) s += g[o + j] * b[o + j];
	s = block_reduce(s, red, false);
	for (int j = threadIdx.x; j < count; j += 256) h[o + j] = (g[o + j] - s) * b[o + j];
}
// rows = dim[0] (1-d: one row)
static int softmax_batch(const ccv_nnc_tensor_t* a) { return tensor_nd(a->info.dim) < 2 ? 1 : a->info.dim[0]; }
static bool is_half(const ccv_nnc_tensor_t* t) { return t && CCV_GET_DATA_TYPE(t->info.datatype) == CCV_16F; }
// CCV_16F tensors (half_stage.cpp g_native_half, tunable ROW_HALF_NATIVE): the row kernels of row_ops.h -- the row in registers, b written once
static int softmax_half(const ccv_nnc_tensor_t* g, const ccv_nnc_tensor_t* ab, ccv_nnc_tensor_t* out, ccv_nnc_stream_context_t* const ctx)
{ // forward: (0, a, b); backward: (g, b, h)
	if (!dense_of(ab, CCV_16F) || !dense_of(out, CCV_16F) || !same_count(ab, out) || (g && (!dense_of(g, CCV_16F) || !same_count(g, ab)))) return CCV_NNC_EXEC_INVALID;
	const ccv_nnc_tensor_t* const first = g ? g : ab;
	const int batch = softmax_batch(first);
	const size_t n = tensor_count(first->info);
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	if (batch < 1 || n / batch > (size_t)rows::ROW_REG_MAX) return CCV_NNC_EXEC_INVALID;
	rows::softmax_args_t p = {};
	p.rows = batch; p.n = (int)(n / batch);
	if (g) { p.g = g->data.u8; p.b_in = ab->data.u8; p.h = out->data.u8; return rows::softmax_bwd<rows::half_t>(p, ctx); }
	p.a = ab->data.u8; p.b = out->data.u8;
	return rows::softmax_fwd<rows::half_t>(p, ctx);
}
static int _softmax_forw(EXEC_ARGS)
{
	if (input_size >= 1 && output_size >= 1 && is_half(inputs[0])) return softmax_half(0, inputs[0], outputs[0], stream_context);
	if (input_size < 1 || output_size < 1 || !dense_f32(inputs[0]) || !dense_f32(outputs[0]) || !same_count(inputs[0], outputs[0])) return CCV_NNC_EXEC_INVALID;
	const ccv_nnc_tensor_t* a = inputs[0];
	const int batch = tensor_nd(a->info.dim) < 2 ? 1 : a->info.dim[0];
	const size_t n = tensor_count(a->info);
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	hipLaunchKernelGGL(softmax_forw_kernel, dim3(batch), dim3(256), 0, stream_of(stream_context), (const float*)a->data.f32, outputs[0]->data.f32, (int)(n / batch));
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}
static int _softmax_back(EXEC_ARGS)
{
	if (input_size >= 3 && output_size >= 1 && is_half(inputs[0])) return softmax_half(inputs[0], inputs[2], outputs[0], stream_context);
	if (input_size < 3 || output_size < 1 || !dense_f32(inputs[0]) || !dense_f32(inputs[2]) || !dense_f32(outputs[0]) || !same_count(inputs[0], inputs[2]) || !same_count(inputs[0], outputs[0])) return CCV_NNC_EXEC_INVALID;
	const ccv_nnc_tensor_t* g = inputs[0];
	const int batch = tensor_nd(g->info.dim) < 2 ? 1 : g->info.dim[0];
	const size_t n = tensor_count(g->info);
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	hipLaunchKernelGGL(softmax_back_kernel, dim3(batch), dim3(256), 0, stream_of(stream_context), (const float*)g->data.f32, (const float*)inputs[2]->data.f32, outputs[0]->data.f32, (int)(n / batch));
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

// ---- optimizers: one pass over (g, a, m, v[, vm]) -> (b, n, u[, um]); the kernels and the arithmetic are optim.h's --------------------------------
// g is CCV_32F or CCV_16F; the parameter and state tensors share one of the two types (what the reference's GPU kernels dispatch on).  CCV_16F tensors arrive
// here only through half_stage.cpp's native rows (tunable OPT_HALF_NATIVE); without them every tensor is an fp32 one or an fp32 image.
// -> 0 and the two types, or the code to return: dense tensors of one element count, g of *tg, the others of *tp
static int opt_tensors(ccv_nnc_tensor_t* const* const inputs, const int nin, ccv_nnc_tensor_t* const* const outputs, const int nout, int* const tg, int* const tp, size_t* const n)
{
	*tg = float_type(inputs[0]);
	*tp = float_type(inputs[1]);
	if (!*tg || !*tp || !dense_of(inputs[0], *tg)) return CCV_NNC_EXEC_INVALID;
	for (int i = 1; i < nin; i++) if (!dense_of(inputs[i], *tp)) return CCV_NNC_EXEC_INVALID;
	for (int i = 0; i < nout; i++) if (!dense_of(outputs[i], *tp)) return CCV_NNC_EXEC_INVALID;
	*n = tensor_count(inputs[1]->info);
	for (int i = 0; i < nin; i++) if (tensor_count(inputs[i]->info) != *n) return CCV_NNC_EXEC_INVALID;
	for (int i = 0; i < nout; i++) if (tensor_count(outputs[i]->info) != *n) return CCV_NNC_EXEC_INVALID;
	return 0;
}
// CALL<TG, TP>() for the pair of element types
#define OPT_DISPATCH(tg, tp, CALL) ((tg) == CCV_16F ? ((tp) == CCV_16F ? CALL(optim::half_t, optim::half_t) : CALL(optim::half_t, float)) : ((tp) == CCV_16F ? CALL(float, optim::half_t) : CALL(float, float)))

static optim::opt_ptrs_t opt_ptrs(ccv_nnc_tensor_t* const* const inputs, const int nin, ccv_nnc_tensor_t* const* const outputs, const int nout)
{
	optim::opt_ptrs_t p = {};
	for (int i = 0; i < nin; i++) p.in[i] = inputs[i]->data.u8;
	for (int i = 0; i < nout; i++) p.out[i] = outputs[i]->data.u8;
	return p;
}
template <bool DECOUPLED, bool AMS>
static int adam_run(const ccv_nnc_cmd_t& cmd, const int tg, const int tp, const optim::opt_ptrs_t& ptrs, const size_t n, ccv_nnc_stream_context_t* const ctx)
{
	optim::AdamOp<DECOUPLED, AMS> p;
	p.scale = cmd.info.adam.scale; p.beta1 = cmd.info.adam.beta1; p.beta2 = cmd.info.adam.beta2; p.decay = cmd.info.adam.decay; p.epsilon = cmd.info.adam.epsilon;
	p.rate_corr1 = cmd.info.adam.rate / (1 - powf(p.beta1, (float)cmd.info.adam.step));
	p.inv_corr2 = 1.f / (1 - powf(p.beta2, (float)cmd.info.adam.step));
	p.rate_decay = cmd.info.adam.rate * p.decay;
	const char* const name = DECOUPLED ? "optim_adamw" : "optim_adam";
#define ADAM_CALL(TG, TP) optim::opt_pass<optim::AdamOp<DECOUPLED, AMS>, TG, TP>(name, p, ptrs, n, ctx)
	return OPT_DISPATCH(tg, tp, ADAM_CALL);
#undef ADAM_CALL
}
static int adam_exec(const ccv_nnc_cmd_t& cmd, const int decoupled, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, ccv_nnc_stream_context_t* const ctx)
{
	if (input_size < 4 || output_size < 3) return CCV_NNC_EXEC_INVALID;
	const ccv_nnc_tensor_t* vm = input_size >= 5 ? inputs[4] : 0;
	ccv_nnc_tensor_t* um = output_size >= 4 ? outputs[3] : 0;
	const int ams = cmd.info.adam.amsgrad && vm && um;
	int tg, tp;
	size_t n;
	const int bad = opt_tensors(inputs, ams ? 5 : 4, outputs, ams ? 4 : 3, &tg, &tp, &n);
	if (bad) return bad;
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	const optim::opt_ptrs_t ptrs = opt_ptrs(inputs, ams ? 5 : 4, outputs, ams ? 4 : 3);
	if (decoupled) return ams ? adam_run<true, true>(cmd, tg, tp, ptrs, n, ctx) : adam_run<true, false>(cmd, tg, tp, ptrs, n, ctx);
	return ams ? adam_run<false, true>(cmd, tg, tp, ptrs, n, ctx) : adam_run<false, false>(cmd, tg, tp, ptrs, n, ctx);
}
static int _adam_forw(EXEC_ARGS) { return adam_exec(cmd, 0, IO); }
static int _adamw_forw(EXEC_ARGS) { return adam_exec(cmd, 1, IO); }

static int _rmsprop_forw(EXEC_ARGS)
{
	if (input_size < 4 || output_size < 3) return CCV_NNC_EXEC_INVALID;
	int tg, tp;
	size_t n;
	const int bad = opt_tensors(inputs, 4, outputs, 3, &tg, &tp, &n);
	if (bad) return bad;
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	const optim::RmspropOp p = { cmd.info.rmsprop.rate, cmd.info.rmsprop.scale, cmd.info.rmsprop.decay, cmd.info.rmsprop.alpha, cmd.info.rmsprop.momentum, cmd.info.rmsprop.epsilon };
	const optim::opt_ptrs_t ptrs = opt_ptrs(inputs, 4, outputs, 3);
#define RMSPROP_CALL(TG, TP) optim::opt_pass<optim::RmspropOp, TG, TP>("optim_rmsprop", p, ptrs, n, stream_context)
	return OPT_DISPATCH(tg, tp, RMSPROP_CALL);
#undef RMSPROP_CALL
}

// ---- LAMB: update = mom^ / (sqrt(vel^) + eps) + decay w; b = a - rate (|w| / |update|) update.  Three launches (optim.h lamb_run): the element pass writes n, u
// and the update (workspace, fp32) and one (sum w^2, sum update^2) pair per workgroup in double; one thread folds the pairs in order into the trust
// ratio; the last pass applies it.  Deterministic. -------------------------------------------------------------------------------------
static int _lamb_forw(EXEC_ARGS)
{
	if (input_size < 4 || output_size < 3) return CCV_NNC_EXEC_INVALID;
	int tg, tp;
	size_t n;
	const int bad = opt_tensors(inputs, 4, outputs, 3, &tg, &tp, &n);
	if (bad) return bad;
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	optim::LambUpdateOp p;
	p.scale = cmd.info.lamb.scale; p.beta1 = cmd.info.lamb.beta1; p.beta2 = cmd.info.lamb.beta2; p.decay = cmd.info.lamb.decay; p.epsilon = cmd.info.lamb.epsilon;
	p.inv_corr1 = 1.f / (1 - powf(p.beta1, (float)cmd.info.lamb.step));
	p.inv_corr2 = 1.f / (1 - powf(p.beta2, (float)cmd.info.lamb.step));
#define LAMB_CALL(TG, TP) optim::lamb_run<TG, TP>(p, cmd.info.lamb.rate, (const TG*)inputs[0]->data.u8, (const TP*)inputs[1]->data.u8, (const TP*)inputs[2]->data.u8, (const TP*)inputs[3]->data.u8, (TP*)outputs[0]->data.u8, (TP*)outputs[1]->data.u8, (TP*)outputs[2]->data.u8, n, stream_context)
	return OPT_DISPATCH(tg, tp, LAMB_CALL);
#undef LAMB_CALL
}

} // namespace

bool nnc::softmax_half_applies(const ccv_nnc_cmd_t cmd, int, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size)
{
	if (!tune(TUNE_ROW_HALF_NATIVE) || input_size < 1 || !inputs[0]) return false;
	const size_t n = tensor_count(inputs[0]->info);
	const int batch = softmax_batch(inputs[0]);
	return batch >= 1 && n / batch <= (size_t)rows::ROW_REG_MAX;
}

#define NNC_REG(CMD, BACKEND, FORMATS, EXEC) \
	extern "C" void _register_command_##CMD##_backend_##BACKEND(ccv_nnc_cmd_backend_registry_t* const registry) \
	{ registry->tensor_formats = (FORMATS); registry->tensor_datatypes = CCV_32F; registry->tensor_memory = CCV_TENSOR_GPU_MEMORY; registry->algorithms = 1; registry->exec = EXEC; NNC_HALF_STAGED(registry, EXEC); }
#define ALL_FORMATS (CCV_TENSOR_FORMAT_NCHW | CCV_TENSOR_FORMAT_NHWC | CCV_TENSOR_FORMAT_CHWN)

NNC_REG(CCV_NNC_SIGMOID_FORWARD, CCV_NNC_BACKEND_GPU_CUDNN, ALL_FORMATS, _sigmoid_forw)
NNC_REG(CCV_NNC_SIGMOID_BACKWARD, CCV_NNC_BACKEND_GPU_CUDNN, ALL_FORMATS, _sigmoid_back)
NNC_REG(CCV_NNC_TANH_FORWARD, CCV_NNC_BACKEND_GPU_CUDNN, ALL_FORMATS, _tanh_forw)
NNC_REG(CCV_NNC_TANH_BACKWARD, CCV_NNC_BACKEND_GPU_CUDNN, ALL_FORMATS, _tanh_back)
NNC_REG(CCV_NNC_GELU_FORWARD, CCV_NNC_BACKEND_GPU_REF, ALL_FORMATS, _gelu_forw)
NNC_REG(CCV_NNC_GELU_BACKWARD, CCV_NNC_BACKEND_GPU_REF, ALL_FORMATS, _gelu_back)
NNC_REG(CCV_NNC_SWISH_FORWARD, CCV_NNC_BACKEND_GPU_REF, ALL_FORMATS, _swish_forw)
NNC_REG(CCV_NNC_SWISH_BACKWARD, CCV_NNC_BACKEND_GPU_REF, ALL_FORMATS, _swish_back)
NNC_REG(CCV_NNC_LEAKY_RELU_FORWARD, CCV_NNC_BACKEND_GPU_REF, ALL_FORMATS, _leaky_forw)
NNC_REG(CCV_NNC_LEAKY_RELU_BACKWARD, CCV_NNC_BACKEND_GPU_REF, ALL_FORMATS, _leaky_back)
NNC_REG(CCV_NNC_SOFTMAX_FORWARD, CCV_NNC_BACKEND_GPU_CUDNN, ALL_FORMATS, _softmax_forw)
NNC_REG(CCV_NNC_SOFTMAX_BACKWARD, CCV_NNC_BACKEND_GPU_CUDNN, ALL_FORMATS, _softmax_back)
NNC_REG(CCV_NNC_ADAM_FORWARD, CCV_NNC_BACKEND_GPU_REF, ALL_FORMATS, _adam_forw)
NNC_REG(CCV_NNC_ADAMW_FORWARD, CCV_NNC_BACKEND_GPU_REF, ALL_FORMATS, _adamw_forw)
NNC_REG(CCV_NNC_RMSPROP_FORWARD, CCV_NNC_BACKEND_GPU_REF, ALL_FORMATS, _rmsprop_forw)
NNC_REG(CCV_NNC_LAMB_FORWARD, CCV_NNC_BACKEND_GPU_REF, ALL_FORMATS, _lamb_forw)
