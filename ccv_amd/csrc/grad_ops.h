// The two passes a trainer makes over every parameter gradient between backward and the optimizer -- gradient clipping by the global norm and the NaN check
// (the reference's ccv_cnnp_model_parameters_clip_grad_norm / ccv_cnnp_model_parameter_gradients_isnan, lib/nnc/ccv_cnnp_model_addons.c) -- on dense CCV_16F
// gradients without fp32 images (cmd_bcast.cpp; tunable GRAD_HALF_NATIVE):
//   REDUCE_NORM2_FORWARD   half [n] -> one CCV_32F or CCV_16F element    sqrt of the sum of squares
//   REDUCE_ISNAN_FORWARD   half [n] -> one CCV_32S element               1 where any element is a NaN, else 0
//   MUL_FORWARD            half [n] x one CCV_32F / CCV_16F element -> half [n], in place or not
//
// The reductions.  Halves are loaded 16 bytes per lane; squares and sums are fp32 (the square of a half is exact there), the NaN test is on the loaded words as
// integers ((bits & 0x7fff) > 0x7c00), nothing is widened.  The elements in front of the first 16-byte boundary (at most 7, a base that is only 2-byte aligned)
// and behind the last whole vector (at most 7) go to the first lanes of workgroup 0 IN THE SAME LAUNCH.
//   up to GRAD_ONE_WG_MAX elements   ONE workgroup walks the tensor and writes the result: one launch (the hundreds of biases and norm scales of a model)
//   above                            a front of workgroups, one tile of GRAD_TILE x GRAD_THREADS vectors each, writes one fp32 (int32) partial per workgroup into the
//                                    stream's workspace; grad_fold_kernel, one workgroup, folds them and writes the result: two launches
// Choice of the geometry (the guides' sections on HBM-bound kernels): a lane has GRAD_TILE = 8 independent 16-byte loads in flight before its first use, a
// workgroup 32 KiB -- the "streaming" load per CU of the microarchitecture guide from ONE resident workgroup, eight times that at full occupancy; the grid covers
// the tensor with one trip per workgroup (a front walking the tensor in order: ew_map.h measured 6.2 TB/s for it against 4.7 TB/s for a capped grid striding
// it), so above the threshold the workgroup count is the tile count, a function of the element count alone.  The threshold is measured (DESIGN.md section 3.2,
// tools/grad_half_bench.py --sweep; a GRAD_HALF_NATIVE above 1 is the threshold in elements, for that measurement): issued back to back, one workgroup finishes
// 131 072 elements (eight trips) inside the 6.5 us a command takes to issue, where two launches take 10 us; at 262 144 elements the lone workgroup takes 11 us and the
// two launches win.  That is the host-bound regime of a stream fed command by command; what the device alone takes (graph replay) is not measured.
// Determinism: every sum has ONE order, fixed by the element count and the base's alignment -- per lane GRAD_TILE accumulators (one per vector slot) folded
// pairwise, per wave a shuffle tree, across waves lane 0 walking LDS in wave order, across workgroups the fold's four strided accumulators per lane and the same
// tree.  No atomics, no zeroing pass (every output is written exactly once), nothing depends on dispatch order: two runs give the same bits.
// The reduce axes of the commands are not consulted: a one-element output says that everything is reduced (as bcast_reduce reads it).
//
// MUL by a one-element tensor: out = f32_rounded((p a) b) in the command's operand order, the bits of cmd_bcast.cpp's FMul followed by a conversion.  The scalar
// stays in device memory and is read by the kernel (the host never sees it: capture and replay keep working).  One launch of ew_map_kernel (ew_map.h) with the
// functor below; out may be the large operand's own memory, every lane reads what it overwrites first.
//
// grad_half_plan is the ONE decision: half_stage.cpp's predicate (grad_half_applies) and the exec functions (grad_half_exec) both call it.
#pragma once
#include "ew_map.h"
#include <math.h>

namespace nnc {

constexpr int GRAD_THREADS = 256;
constexpr int GRAD_TILE = 8; // 16-byte vectors per lane and trip: a workgroup takes GRAD_TILE * GRAD_THREADS vectors (32 KiB) per trip
constexpr int GRAD_ONE_WG_MAX = 131072; // elements up to which one workgroup does the whole reduction (eight tiles)
constexpr int GRAD_FOLD_THREADS = 1024;
constexpr double GRAD_MAX_ELEMENTS = 2147483648.0; // 2^31 elements and more keep their route

enum { GRAD_NORM2 = 0, GRAD_ISNAN = 1, GRAD_SCALE = 2 };

// ---- geometry and plan ---------------------------------------------------------------------------------------------------------------------------------------
// x[0 .. head) in front of the first 16-byte boundary, nv whole vectors from x + head, the rest behind them: head + (n - head - 8 nv) <= 14 edge elements
struct grad_geom_t { unsigned n, head, nv, blocks, trips; };
static inline grad_geom_t grad_geometry(const void* const x, const unsigned n)
{
	grad_geom_t g;
	g.n = n;
	g.head = (unsigned)(((16 - ((uintptr_t)x & 15)) & 15) / sizeof(half_t));
	if (g.head > n) g.head = n;
	g.nv = (n - g.head) / 8;
	const unsigned tiles = (g.nv + GRAD_TILE * GRAD_THREADS - 1) / (GRAD_TILE * GRAD_THREADS);
	const long key = tune(TUNE_GRAD_HALF_NATIVE); // above 1: the threshold itself, in elements (measurements: tools/grad_half_bench.py --sweep)
	const bool one = n <= (key > 1 ? (unsigned long)key : (unsigned long)GRAD_ONE_WG_MAX);
	g.blocks = one || tiles < 1 ? 1 : tiles;
	g.trips = one ? tiles : 1;
	return g;
}

struct grad_plan_t {
	int kind;
	unsigned n;       // elements of the half tensor
	const half_t* x;  // the half tensor read
	void* out;        // reductions: the one element written;  MUL: the half tensor written
	int out_half;     // NORM2: the result is a half
	const void* s;    // MUL: the one-element tensor
	int s_half, first; // ... a half; it is the command's first operand
	float p;
};

static inline bool grad_dense(const ccv_nnc_tensor_t* t, const int datatype) { return t && !CCV_IS_TENSOR_VIEW(t) && CCV_GET_DATA_TYPE(t->info.datatype) == datatype && t->data.u8; }
static inline bool grad_scalar(const ccv_nnc_tensor_t* t, const int dt0, const int dt1) { return (grad_dense(t, dt0) || grad_dense(t, dt1)) && tensor_count(t->info) == 1; }
// mul_planes.h's squeeze-excite pattern at N = C = 1: a 4-d tensor of one image and one channel by a 4-d one-element tensor of its type and format.  That pattern
// has a key of its own (MUL_PLANES) whose 0 says "the generic kernels": it is not taken here
static inline bool grad_plane_scale(const ccv_nnc_tensor_t* big, const ccv_nnc_tensor_t* small)
{
	if (tensor_nd(big->info.dim) != 4 || tensor_nd(small->info.dim) != 4 || big->info.datatype != small->info.datatype || big->info.format != small->info.format) return false;
	return big->info.dim[0] == 1 && big->info.dim[big->info.format == CCV_TENSOR_FORMAT_NHWC ? 3 : 1] == 1;
}
static inline bool grad_overlap(const void* a, const size_t na, const void* b, const size_t nb) { return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na; }
// true: the key is on, nothing is accumulated and
//   REDUCE_NORM2_FORWARD  input 0 is a dense CCV_16F tensor of 1 .. 2^31 - 1 elements, output 0 a dense one-element CCV_32F or CCV_16F tensor
//   REDUCE_ISNAN_FORWARD  the same with a CCV_32S output
//   MUL_FORWARD           one operand and the output are dense CCV_16F tensors of one element count (1 .. 2^31 - 1), the other operand is a dense one-element CCV_32F
//                         or CCV_16F tensor; the output meets the large operand's memory only as the same memory, and the scalar's not at all; the command is
//                         not of mul_planes.h's pattern (grad_plane_scale)
// -- *o then holds the launch.  false: the command keeps today's route (partial-axis reductions, views, accumulation, other types).
static bool grad_half_plan(const ccv_nnc_cmd_t cmd, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, grad_plan_t* const o)
{
	if (!tune(TUNE_GRAD_HALF_NATIVE) || (flags & CCV_NNC_ACCUMULATE_OUTPUT) || input_size < 1 || output_size < 1 || !outputs[0]) return false;
	memset(o, 0, sizeof(*o));
	ccv_nnc_tensor_t* const out = outputs[0];
	if (cmd.cmd == CCV_NNC_REDUCE_NORM2_FORWARD || cmd.cmd == CCV_NNC_REDUCE_ISNAN_FORWARD) {
		const ccv_nnc_tensor_t* const x = inputs[0];
		if (!grad_dense(x, CCV_16F)) return false;
		const size_t n = tensor_count(x->info);
		if (n < 1 || (double)n >= GRAD_MAX_ELEMENTS) return false;
		if (cmd.cmd == CCV_NNC_REDUCE_NORM2_FORWARD ? !grad_scalar(out, CCV_32F, CCV_16F) : !grad_scalar(out, CCV_32S, CCV_32S)) return false;
		o->kind = cmd.cmd == CCV_NNC_REDUCE_NORM2_FORWARD ? GRAD_NORM2 : GRAD_ISNAN;
		o->n = (unsigned)n; o->x = (const half_t*)x->data.u8; o->out = out->data.u8;
		o->out_half = CCV_GET_DATA_TYPE(out->info.datatype) == CCV_16F;
		return !grad_overlap(o->x, sizeof(half_t) * n, o->out, 4);
	}
	if (cmd.cmd != CCV_NNC_MUL_FORWARD || input_size < 2 || !grad_dense(out, CCV_16F)) return false;
	const size_t n = tensor_count(out->info);
	if (n < 1 || (double)n >= GRAD_MAX_ELEMENTS) return false;
	for (int k = 0; k < 2; k++) { // the large operand first, then second
		const ccv_nnc_tensor_t* const big = inputs[k];
		const ccv_nnc_tensor_t* const small = inputs[1 - k];
		if (!grad_dense(big, CCV_16F) || tensor_count(big->info) != n || !grad_scalar(small, CCV_32F, CCV_16F) || grad_plane_scale(big, small)) continue;
		o->kind = GRAD_SCALE;
		o->n = (unsigned)n; o->x = (const half_t*)big->data.u8; o->out = out->data.u8; o->s = small->data.u8;
		o->s_half = CCV_GET_DATA_TYPE(small->info.datatype) == CCV_16F; o->first = k; o->p = cmd.info.blas.a[0];
		if (o->out != (const void*)o->x && grad_overlap(o->out, sizeof(half_t) * n, o->x, sizeof(half_t) * n)) return false;
		return !grad_overlap(o->out, sizeof(half_t) * n, o->s, o->s_half ? sizeof(half_t) : sizeof(float));
	}
	return false;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------------------------------------
typedef unsigned grad_u32x4 __attribute__((ext_vector_type(4)));
template <int OP> struct grad_red;
template <> struct grad_red<GRAD_NORM2> {
	typedef float T;
	typedef pack16<half_t>::type V;
	static __device__ __forceinline__ T comb(const T a, const T b) { return a + b; }
	static __device__ __forceinline__ T one(const half_t h) { return (float)h * (float)h; }
	static __device__ __forceinline__ T vec(const V v)
	{
		float s = 0.f;
#pragma unroll
		for (int e = 0; e < 8; e++) s += (float)v[e] * (float)v[e];
		return s;
	}
	static __device__ __forceinline__ void finish(const T s, void* const out, const int out_half)
	{
		const float r = sqrtf(s);
		if (out_half) *(half_t*)out = (half_t)f32_rounded(r); // the one rounding to half
		else *(float*)out = r;
	}
};
template <> struct grad_red<GRAD_ISNAN> {
	typedef unsigned T;
	typedef pack16<half_t>::type V;
	static __device__ __forceinline__ T comb(const T a, const T b) { return a | b; }
	static __device__ __forceinline__ T one(const half_t h) { return (unsigned)((__builtin_bit_cast(unsigned short, h) & 0x7fffu) > 0x7c00u); }
	static __device__ __forceinline__ T vec(const V v)
	{
		const grad_u32x4 w = __builtin_bit_cast(grad_u32x4, v); // two halves per word
		unsigned s = 0;
#pragma unroll
		for (int d = 0; d < 4; d++) s |= (unsigned)((w[d] & 0x7fffu) > 0x7c00u) | (unsigned)(((w[d] >> 16) & 0x7fffu) > 0x7c00u);
		return s;
	}
	static __device__ __forceinline__ void finish(const T s, void* const out, int) { *(int*)out = s ? 1 : 0; }
};

// the workgroup's value in thread 0: a shuffle tree per wave, then lane 0 walks the waves' values in wave order
template <int OP>
__device__ __forceinline__ typename grad_red<OP>::T grad_workgroup(typename grad_red<OP>::T s)
{
	typedef grad_red<OP> R;
	__shared__ typename R::T red[GRAD_FOLD_THREADS / 64];
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) s = R::comb(s, __shfl_down(s, off, 64));
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
	__syncthreads();
	if (threadIdx.x == 0)
		for (unsigned w = 1; w < (blockDim.x >> 6); w++) s = R::comb(s, red[w]);
	return s;
}

// Workgroup b takes the tiles b * trips .. b * trips + trips - 1 of the nv vectors that start at x + head; workgroup 0 the edge elements as well.  One workgroup
// (gridDim.x == 1) writes the result, several write partial[b].
template <int OP>
__global__ void __launch_bounds__(GRAD_THREADS) grad_reduce_kernel(const half_t* x, const unsigned n, const unsigned head, const unsigned nv, const unsigned trips, typename grad_red<OP>::T* partial, void* out, const int out_half)
{
	typedef grad_red<OP> R;
	typedef typename R::V V;
	typedef typename R::T T;
	const V* const xv = (const V*)(x + head);
	T acc[GRAD_TILE];
#pragma unroll
	for (int u = 0; u < GRAD_TILE; u++) acc[u] = T(0);
	for (unsigned t = 0; t < trips; t++) {
		const unsigned base = (blockIdx.x * trips + t) * (GRAD_TILE * GRAD_THREADS) + threadIdx.x;
		V v[GRAD_TILE];
#pragma unroll
		for (int u = 0; u < GRAD_TILE; u++) {
			const unsigned i = base + u * GRAD_THREADS;
			v[u] = i < nv ? xv[i] : V{}; // (zeros add nothing to either reduction)
		}
#pragma unroll
		for (int u = 0; u < GRAD_TILE; u++) acc[u] = R::comb(acc[u], R::vec(v[u]));
	}
	const unsigned tail = n - head - nv * 8;
	if (blockIdx.x == 0 && threadIdx.x < head + tail) acc[0] = R::comb(acc[0], R::one(x[threadIdx.x < head ? threadIdx.x : n - tail + (threadIdx.x - head)]));
	const T s = grad_workgroup<OP>(R::comb(R::comb(R::comb(acc[0], acc[1]), R::comb(acc[2], acc[3])), R::comb(R::comb(acc[4], acc[5]), R::comb(acc[6], acc[7]))));
	if (threadIdx.x != 0) return;
	if (gridDim.x == 1) R::finish(s, out, out_half);
	else partial[blockIdx.x] = s;
}
static_assert(GRAD_TILE == 8, "grad_reduce_kernel folds eight accumulators by name");

// one workgroup: lane t adds partial[t], partial[t + THREADS], ... with four accumulators, then the workgroup's tree
template <int OP>
__global__ void __launch_bounds__(GRAD_FOLD_THREADS) grad_fold_kernel(const typename grad_red<OP>::T* partial, const unsigned count, void* out, const int out_half)
{
	typedef grad_red<OP> R;
	typedef typename R::T T;
	T acc[4] = { T(0), T(0), T(0), T(0) };
	for (unsigned i = threadIdx.x; i < count; i += 4 * GRAD_FOLD_THREADS) {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const unsigned j = i + k * GRAD_FOLD_THREADS;
			if (j < count) acc[k] = R::comb(acc[k], partial[j]);
		}
	}
	const T s = grad_workgroup<OP>(R::comb(R::comb(acc[0], acc[1]), R::comb(acc[2], acc[3])));
	if (threadIdx.x == 0) R::finish(s, out, out_half);
}

// MUL by the one-element tensor s (ew_map_kernel's one-operand form): a is the large operand's element
struct GScale {
	float p;
	const void* s;
	int s_half, first;
	__device__ float operator()(float a, float, float) const
	{
		const float v = s_half ? (float)*(const half_t*)s : *(const float*)s;
		return f32_rounded(first ? (p * v) * a : (p * a) * v); // FMul's operand order
	}
};

// ---- launchers -----------------------------------------------------------------------------------------------------------------------------------------------
// the launch records: "grad_norm2|nnc::grad_reduce_kernel<NORM2>" (+ "grad_norm2|nnc::grad_fold_kernel<NORM2>" above the threshold), the same with isnan / ISNAN,
// "grad_mul|nnc::ew_map_kernel<GScale>"
template <int OP>
static int grad_reduce_run(const grad_plan_t& p, ccv_nnc_stream_context_t* ctx)
{
	typedef typename grad_red<OP>::T T;
	const grad_geom_t g = grad_geometry(p.x, p.n);
	T* partial = 0;
	if (g.blocks > 1 && !(partial = (T*)workspace_of(ctx, sizeof(T) * g.blocks))) return CCV_NNC_EXEC_OOM;
	hipStream_t stream = stream_of(ctx);
	{
		note_kernel(OP == GRAD_NORM2 ? "grad_norm2" : "grad_isnan");
		ProfScope prof(OP == GRAD_NORM2 ? "grad_norm2|nnc::grad_reduce_kernel<NORM2>" : "grad_isnan|nnc::grad_reduce_kernel<ISNAN>", OP == GRAD_NORM2 ? 2. * p.n : (double)p.n, sizeof(half_t) * (double)p.n + 4. * (g.blocks > 1 ? g.blocks : 1), (int)p.n, (int)g.blocks, (int)g.trips, 1, 1, stream);
		hipLaunchKernelGGL(HIP_KERNEL_NAME(grad_reduce_kernel<OP>), dim3(g.blocks), dim3(GRAD_THREADS), 0, stream, p.x, g.n, g.head, g.nv, g.trips, partial, p.out, p.out_half);
		HIP_ENFORCE(hipGetLastError());
	}
	if (g.blocks > 1) {
		note_kernel(OP == GRAD_NORM2 ? "grad_norm2_fold" : "grad_isnan_fold");
		ProfScope prof(OP == GRAD_NORM2 ? "grad_norm2|nnc::grad_fold_kernel<NORM2>" : "grad_isnan|nnc::grad_fold_kernel<ISNAN>", (double)g.blocks, 4. * g.blocks + 4., (int)g.blocks, 1, 1, 1, 1, stream);
		hipLaunchKernelGGL(HIP_KERNEL_NAME(grad_fold_kernel<OP>), dim3(1), dim3(GRAD_FOLD_THREADS), 0, stream, (const T*)partial, g.blocks, p.out, p.out_half);
		HIP_ENFORCE(hipGetLastError());
	}
	return CCV_NNC_EXEC_SUCCESS;
}
static int grad_half_run(const grad_plan_t& p, ccv_nnc_stream_context_t* ctx)
{
	if (p.kind == GRAD_NORM2) return grad_reduce_run<GRAD_NORM2>(p, ctx);
	if (p.kind == GRAD_ISNAN) return grad_reduce_run<GRAD_ISNAN>(p, ctx);
	GScale f;
	f.p = p.p; f.s = p.s; f.s_half = p.s_half; f.first = p.first;
	note_kernel("grad_mul");
	ProfScope prof("grad_mul|nnc::ew_map_kernel<GScale>", 2. * p.n, 2. * sizeof(half_t) * (double)p.n + (p.s_half ? 2. : 4.), (int)p.n, 1, 1, 1, 1, stream_of(ctx));
	return ew_map<GScale, 1, half_t>(f, (half_t*)p.out, p.x, (const half_t*)0, (const half_t*)0, p.n, ctx);
}

} // namespace nnc
