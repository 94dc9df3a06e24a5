// The element passes of RMSPROP, ADAM / ADAMW and LAMB over tensors of two element types: TG for the gradient g, TP for the parameter and state tensors
// (a, m, v[, vm] -> b, n, u[, um]; the reference asserts that these share one type).  Each is float or _Float16 -- the four cases the reference's GPU
// kernels dispatch on (lib/nnc/cmd/rmsprop/gpu/ccv_nnc_rmsprop_gpu_ref.cu:63-74 and its ADAM / ADAMW / LAMB siblings): all fp32, all half, half gradients into
// fp32 master parameters, fp32 gradients into half state.
//
// Arithmetic: ONE functor per optimizer over float values (RmspropOp, AdamOp, LambUpdateOp, LambApplyOp), called by every instantiation: operands are widened
// on load (exact), every stored value is rounded to fp32 by the arithmetic and then once more by the store's conversion (f32_rounded, common.h) -- the bits
// an fp32 kernel between converting passes gives.  No transcendentals; division and square root are correctly rounded.
// Memory: a workgroup takes one contiguous tile of OPT_TILE elements over a full grid.  With every base 16-byte aligned a lane takes
// OPT_LANE = 8 consecutive elements of every tensor -- one 16-byte load for a half operand, two for an fp32 one -- and issues all of its loads before the
// first use; the tail (n mod 8 elements), or everything when a base is not aligned, goes one element per lane.  A lane reads all of its elements before it
// writes any and no lane touches another lane's elements: outputs may be the inputs themselves (b = a, n = m, u = v, um = vm), as the host issues them.
// No scratch beyond LAMB's update image and its per-workgroup norm pairs.
#pragma once
#include "common.h"

namespace nnc {
namespace optim {

constexpr int OPT_THREADS = 256;
constexpr int OPT_LANE = 8;
constexpr int OPT_TILE = 2048; // elements of one workgroup's tile (tests/test_optim_half.py reads this line)
static_assert(OPT_TILE == OPT_THREADS * OPT_LANE, "a lane per OPT_LANE elements");
constexpr int OPT_MAX_IN = 5, OPT_MAX_OUT = 4;

typedef _Float16 half_t;
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float float4_t __attribute__((ext_vector_type(4)));

// eight consecutive elements as they lie in memory: loaded whole, widened afterwards
template <class T> struct raw8;
template <> struct raw8<float> {
	float4_t lo, hi;
	__device__ __forceinline__ void load(const float* p) { lo = ((const float4_t*)p)[0]; hi = ((const float4_t*)p)[1]; }
	__device__ __forceinline__ float get(const int e) const { return e < 4 ? lo[e] : hi[e - 4]; }
	__device__ __forceinline__ void set(const int e, const float v) { if (e < 4) lo[e] = v; else hi[e - 4] = v; }
	__device__ __forceinline__ void store(float* p) const { ((float4_t*)p)[0] = lo; ((float4_t*)p)[1] = hi; }
};
template <> struct raw8<half_t> {
	half8_t v;
	__device__ __forceinline__ void load(const half_t* p) { v = *(const half8_t*)p; }
	__device__ __forceinline__ float get(const int e) const { return (float)v[e]; }
	__device__ __forceinline__ void set(const int e, const float x) { v[e] = (half_t)x; }
	__device__ __forceinline__ void store(half_t* p) const { *(half8_t*)p = v; }
};

// ---- the arithmetic: x = (g, a, m, v[, vm]) -> y = (b, n, u[, um]) -------------------------------------------------------------------------
// Contraction is spelled out, not left to the compiler: with it on, which multiplies and adds become one fma depends on how the vectorizer packs the
// surrounding code, and the scalar loop, the 8-element lanes and the four type instantiations came out differently (seen in the gfx950 assembly).  So the
// pragma turns it off and every fma below is written as one -- exactly those the fp32 kernels these replace were compiled with, whose bits the fp32 / fp32
// instances therefore keep.
struct RmspropOp {
	float rate, scale, decay, alpha, momentum, epsilon;
	static constexpr int NIN = 4, NOUT = 3;
	__device__ __forceinline__ void operator()(const float* const x, float* const y) const
	{
#pragma clang fp contract(off)
		const float av = x[1];
		const float grad = __builtin_fmaf(decay, av, scale * x[0]);
		const float vel = alpha * x[3] + (1.f - alpha) * grad * grad;
		const float mom = __builtin_fmaf(momentum, x[2], grad / (sqrtf(vel) + epsilon));
		y[2] = vel;
		y[1] = mom;
		y[0] = __builtin_fmaf(-rate, mom, av);
	}
};
// ADAM: L2 decay inside the gradient; ADAMW (DECOUPLED): b = a - rate decay a - ...
template <bool DECOUPLED, bool AMS>
struct AdamOp {
	float scale, beta1, beta2, decay, epsilon, rate_corr1, inv_corr2, rate_decay;
	static constexpr int NIN = AMS ? 5 : 4, NOUT = AMS ? 4 : 3;
	__device__ __forceinline__ void operator()(const float* const x, float* const y) const
	{
#pragma clang fp contract(off)
		const float av = x[1];
		float grad = scale * x[0];
		if (!DECOUPLED) grad = __builtin_fmaf(decay, av, grad);
		const float mom = __builtin_fmaf(beta1, x[2], (1.f - beta1) * grad);
		const float vel = __builtin_fmaf(beta2, x[3], (1.f - beta2) * grad * grad);
		y[1] = mom;
		y[2] = vel;
		float denom;
		if (AMS) {
			const float vel_max_hat = fmaxf(x[4], vel * inv_corr2);
			y[3] = vel_max_hat;
			denom = sqrtf(vel_max_hat) + epsilon;
		} else
			denom = sqrtf(vel * inv_corr2) + epsilon;
		const float base = DECOUPLED ? __builtin_fmaf(-rate_decay, av, av) : av;
		y[0] = base - (mom * rate_corr1) / denom;
	}
};
// LAMB, first pass: x = (g, a, m, v) -> y = (update, n, u); the update stays fp32 (workspace)
struct LambUpdateOp {
	float scale, beta1, beta2, decay, epsilon, inv_corr1, inv_corr2;
	__device__ __forceinline__ void operator()(const float* const x, float* const y) const
	{
#pragma clang fp contract(off)
		const float grad = scale * x[0], w = x[1];
		const float mom = __builtin_fmaf(1.f - beta1, grad, beta1 * x[2]);
		const float vel = beta2 * x[3] + (1.f - beta2) * grad * grad;
		y[1] = mom;
		y[2] = vel;
		y[0] = (mom * inv_corr1) / (sqrtf(vel * inv_corr2) + epsilon) + w * decay;
	}
};
// LAMB, last pass: x = (update [fp32], a) -> b
struct LambApplyOp {
	const float* rate_trust;
	static constexpr int NIN = 2, NOUT = 1;
	__device__ __forceinline__ void operator()(const float* const x, float* const y) const { y[0] = __builtin_fmaf(-*rate_trust, x[0], x[1]); }
};

struct opt_ptrs_t { const void* in[OPT_MAX_IN]; void* out[OPT_MAX_OUT]; };

// ---- one pass: in[0] of TG, in[1 ..] and every output of TP.  nv = whole 8-element chunks taken as vectors (0 when a base is not 16-byte aligned) ------
template <class OP, class TG, class TP>
__global__ void __launch_bounds__(OPT_THREADS) opt_pass_kernel(const OP op, const opt_ptrs_t p, const size_t nv, const size_t n)
{
	const size_t c = (size_t)blockIdx.x * OPT_THREADS + threadIdx.x;
	if (c < nv) {
		const size_t o = c * OPT_LANE;
		raw8<TG> g;
		raw8<TP> s[OPT_MAX_IN], r[OPT_MAX_OUT];
		g.load((const TG*)p.in[0] + o);
#pragma unroll
		for (int k = 1; k < OP::NIN; k++) s[k].load((const TP*)p.in[k] + o);
#pragma unroll
		for (int e = 0; e < OPT_LANE; e++) {
			float x[OPT_MAX_IN], y[OPT_MAX_OUT];
			x[0] = g.get(e);
#pragma unroll
			for (int k = 1; k < OP::NIN; k++) x[k] = s[k].get(e);
			op(x, y);
#pragma unroll
			for (int k = 0; k < OP::NOUT; k++) r[k].set(e, f32_rounded(y[k]));
		}
#pragma unroll
		for (int k = 0; k < OP::NOUT; k++) r[k].store((TP*)p.out[k] + o);
	}
	const size_t stride = (size_t)gridDim.x * OPT_THREADS;
	for (size_t j = nv * OPT_LANE + c; j < n; j += stride) {
		float x[OPT_MAX_IN], y[OPT_MAX_OUT];
		x[0] = (float)((const TG*)p.in[0])[j];
#pragma unroll
		for (int k = 1; k < OP::NIN; k++) x[k] = (float)((const TP*)p.in[k])[j];
		op(x, y);
#pragma unroll
		for (int k = 0; k < OP::NOUT; k++) ((TP*)p.out[k])[j] = (TP)f32_rounded(y[k]);
	}
}

static inline bool opt_aligned(const opt_ptrs_t& p, const int nin, const int nout)
{
	for (int k = 0; k < nin; k++) if (!aligned16(p.in[k])) return false;
	for (int k = 0; k < nout; k++) if (!aligned16(p.out[k])) return false;
	return true;
}
// "hh" all half, "hf" half g / fp32 state, "fh" fp32 g / half state, "ff" all fp32: the suffix of the launch records
template <class TG, class TP> static inline const char* opt_type_tag(void) { return sizeof(TG) == 2 ? (sizeof(TP) == 2 ? "hh" : "hf") : (sizeof(TP) == 2 ? "fh" : "ff"); }

// `name`: "optim_rmsprop", "optim_adam", ...; the pointers are dense tensors of n elements each
template <class OP, class TG, class TP>
static int opt_pass(const char* const name, const OP& op, const opt_ptrs_t& p, const size_t n, ccv_nnc_stream_context_t* const ctx)
{
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	const size_t nv = opt_aligned(p, OP::NIN, OP::NOUT) ? n / OPT_LANE : 0;
	size_t blocks = nv ? (nv + OPT_THREADS - 1) / OPT_THREADS : (n + OPT_THREADS - 1) / OPT_THREADS; // (the tail of an aligned tensor is at most 7 elements: the first lanes of workgroup 0)
	if (blocks > 0x7fffffffUL) blocks = 0x7fffffffUL; // (only the scalar loop can be this long, and it strides)
	hipStream_t stream = stream_of(ctx);
	char prof_name[96];
	snprintf(prof_name, sizeof(prof_name), "%s_%s|nnc::optim::opt_pass_kernel", name, opt_type_tag<TG, TP>());
	note_kernel(name);
	ProfScope prof(prof_name, 12.0 * (double)n, (double)n * (sizeof(TG) + sizeof(TP) * (double)(OP::NIN - 1 + OP::NOUT)), (int)(n > 0x7fffffff ? 0x7fffffff : n), 1, 1, 1, 1, stream);
	hipLaunchKernelGGL(HIP_KERNEL_NAME(opt_pass_kernel<OP, TG, TP>), dim3((unsigned)blocks), dim3(OPT_THREADS), 0, stream, op, p, nv, n);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

// ---- LAMB: b = a - rate (|w| / |update|) update, the norms over the whole tensor in double.  Three launches: the update pass (n, u in TP, the update as fp32
// in the workspace, one (sum w^2, sum update^2) pair per workgroup), one thread folding the pairs IN ORDER into rate * trust, the apply pass (opt_pass_kernel with
// LambApplyOp).  A workgroup of the update pass walks `per_wg` consecutive chunks (a multiple of OPT_THREADS: whole tiles), so that the pairs one thread has to
// fold stay few on a large tensor; which elements meet in which pair, and in what order, depends on n and the CU count alone -- the same bits every run, no atomics.
template <class TG, class TP>
__global__ void __launch_bounds__(OPT_THREADS) lamb_update_kernel(const LambUpdateOp op, const TG* g, const TP* a, const TP* m, const TP* v, TP* nm, TP* u, float* update, double* partial, const size_t nv, const size_t n, const size_t per_wg)
{
	__shared__ double red[2][OPT_THREADS / 64];
	double wn = 0, un = 0;
	const size_t first = (size_t)blockIdx.x * per_wg, last = first + per_wg < nv ? first + per_wg : nv;
	for (size_t c = first + threadIdx.x; c < last; c += OPT_THREADS) {
		const size_t o = c * OPT_LANE;
		raw8<TG> rg;
		raw8<TP> ra, rm, rv, on, ou;
		raw8<float> oupd;
		rg.load(g + o); ra.load(a + o); rm.load(m + o); rv.load(v + o);
#pragma unroll
		for (int e = 0; e < OPT_LANE; e++) {
			const float x[4] = { rg.get(e), ra.get(e), rm.get(e), rv.get(e) };
			float y[3];
			op(x, y);
			const float upd = f32_rounded(y[0]);
			oupd.set(e, upd); on.set(e, f32_rounded(y[1])); ou.set(e, f32_rounded(y[2]));
			wn += (double)(x[1] * x[1]);
			un += (double)(upd * upd);
		}
		on.store(nm + o); ou.store(u + o); oupd.store(update + o);
	}
	const size_t stride = (size_t)gridDim.x * OPT_THREADS;
	for (size_t j = nv * OPT_LANE + (size_t)blockIdx.x * OPT_THREADS + threadIdx.x; j < n; j += stride) {
		const float x[4] = { (float)g[j], (float)a[j], (float)m[j], (float)v[j] };
		float y[3];
		op(x, y);
		const float upd = f32_rounded(y[0]);
		nm[j] = (TP)f32_rounded(y[1]);
		u[j] = (TP)f32_rounded(y[2]);
		update[j] = upd;
		wn += (double)(x[1] * x[1]);
		un += (double)(upd * upd);
	}
	for (int o = 32; o > 0; o >>= 1) { wn += __shfl_xor(wn, o); un += __shfl_xor(un, o); }
	if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = wn; red[1][threadIdx.x >> 6] = un; }
	__syncthreads();
	if (threadIdx.x == 0) {
		partial[2 * blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
		partial[2 * blockIdx.x + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
	}
}
static __global__ void lamb_trust_kernel(const double* partial, const int blocks, const float rate, float* rate_trust)
{
	double wn = 0, un = 0;
	for (int i = 0; i < blocks; i++) { wn += partial[2 * i]; un += partial[2 * i + 1]; }
	wn = sqrt(wn); un = sqrt(un);
	const float trust = (wn > 0 && un > 0) ? (float)(wn / un) : 1.f;
	*rate_trust = rate * trust;
}

template <class TG, class TP>
static int lamb_run(const LambUpdateOp& op, const float rate, const TG* g, const TP* a, const TP* m, const TP* v, TP* b, TP* nm, TP* u, const size_t n, ccv_nnc_stream_context_t* const ctx)
{
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	const size_t cap = (size_t)device_cu_count() * 8; // partial pairs at most
	const bool vec = aligned16(g) && aligned16(a) && aligned16(m) && aligned16(v) && aligned16(nm) && aligned16(u);
	const size_t nv = vec ? n / OPT_LANE : 0;
	size_t per_wg = OPT_THREADS, blocks;
	if (nv) {
		const size_t tiles = (nv + OPT_THREADS - 1) / OPT_THREADS;
		per_wg = ((tiles + cap - 1) / cap) * OPT_THREADS;
		blocks = (nv + per_wg - 1) / per_wg;
	} else {
		blocks = (n + OPT_THREADS - 1) / OPT_THREADS;
		if (blocks > cap) blocks = cap;
	}
	const size_t head = (sizeof(double) * 2 * blocks + sizeof(float) + 255) & ~(size_t)255;
	char* const ws = (char*)workspace_of(ctx, head + sizeof(float) * n);
	if (!ws) return CCV_NNC_EXEC_OOM;
	double* const partial = (double*)ws;
	float* const rate_trust = (float*)(ws + sizeof(double) * 2 * blocks);
	float* const update = (float*)(ws + head);
	if (nv && !aligned16(update)) return CCV_NNC_EXEC_INVALID; // (the workspace is 256-byte aligned)
	hipStream_t stream = stream_of(ctx);
	char prof_name[96];
	snprintf(prof_name, sizeof(prof_name), "optim_lamb_%s|nnc::optim::lamb_update_kernel", opt_type_tag<TG, TP>());
	{
		note_kernel("optim_lamb");
		ProfScope prof(prof_name, 14.0 * (double)n, (double)n * (sizeof(TG) + 5.0 * sizeof(TP) + sizeof(float)), (int)(n > 0x7fffffff ? 0x7fffffff : n), 1, 1, 1, (int)blocks, stream);
		hipLaunchKernelGGL(HIP_KERNEL_NAME(lamb_update_kernel<TG, TP>), dim3((unsigned)blocks), dim3(OPT_THREADS), 0, stream, op, g, a, m, v, nm, u, update, partial, nv, n, per_wg);
		hipLaunchKernelGGL(lamb_trust_kernel, dim3(1), dim3(1), 0, stream, (const double*)partial, (int)blocks, rate, rate_trust);
		HIP_ENFORCE(hipGetLastError());
	}
	LambApplyOp apply = { rate_trust };
	opt_ptrs_t p = {};
	p.in[0] = update; p.in[1] = a; p.out[0] = b;
	return opt_pass<LambApplyOp, float, TP>("optim_lamb_apply", apply, p, n, ctx);
}

} // namespace optim
} // namespace nnc
