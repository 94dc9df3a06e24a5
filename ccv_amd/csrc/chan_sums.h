// Column and channel sums: out[c] (+)= the sum of everything in column / channel c.  Every bias gradient (GEMM, convolution, LSTM), the layer-norm and
// RMS-norm parameter gradients and the batch-norm statistics end here.
//
// One scheme throughout, two deterministic stages: per-slice (per-plane) fp32 partials go to the BASE of the stream workspace, a 16 x 16 fold
// (common.h: fold_slices / fold_phases) adds them in a fixed order.  What lives here:
//   * the slice plan of the row forms (colsum_plan) and, next to it, what each form asks of the workspace -- a caller that keeps data of its own
//     behind the partials takes its head size from these functions, never from a restatement of the plan;
//   * the kernel templates: rows (lanes = 64 consecutive columns), planes (a wave per plane), the fold (fp32 or half output, an optional second array);
//   * chan_reduce, the launcher over a [outer][C][inner] view with the batch-norm functors (cmd_norm.cpp uses it with all three);
//   * the per-image column sums of a product of two tensors (scaled_rows_image_kernel: MUL's gradient towards a per-(image, channel) operand, mul_planes.h);
//   * what bcast_ops.h adds to them: the per-image column sums of ONE tensor (rows_image_sum: the NHWC global average pool), and planes by their length
//     (chan_reduce_planes_sliced: sixteen lanes per short plane, a wave per plane, long planes of a launch that would starve cut into slices);
//   * chan_sums.cpp: the 16-byte float rows kernel, the grouped level for thousands of slices, and the five exported sums declared in common.h.
// The route decides the order of the additions and so the bits: see each launcher for which kernel it takes when.
#pragma once
#include "common.h"

namespace nnc {

typedef _Float16 half_t;

// ---- the plan and the workspace each form takes ------------------------------------------------------------------------------------------------------
// rows x cols, columns contiguous: 64-column tiles x row slices, about four workgroups per CU, no slice under 64 rows, none empty.
struct colsum_plan_t { int col_tiles; long slices, rows_per_slice; };
colsum_plan_t colsum_plan(long rows, int cols);
size_t colsum_workspace_bytes(long rows, int cols); // what colsum_f32 / colsum_f16 / chan_reduce (inner == 1) request for this shape
size_t colsum_workspace_bound(int cols); // the most they request for `cols` columns, whatever the rows
size_t colsum_partials_bytes(long slices, int cols); // what colsum_partials_f16's caller provides: its partials and room for the grouped level behind them
inline size_t chan_planes_workspace_bytes(const long outer, const int C) { return sizeof(float) * (size_t)outer * (size_t)C; } // inner > 1: one partial per plane
// Long planes, few of them (the sum of a whole tensor to one value is ONE plane): a wave per plane starves the chip.  A plane longer than CHAN_RUN_SLICE elements is
// cut into at most ceil(inner / CHAN_RUN_SLICE) slices (each a multiple of eight elements, so that a slice starts as aligned as its plane) until the launch has
// CHAN_SLICE_WAVES_PER_CU waves per CU; a wave per slice, partial[o][slice][c], the same fold over outer * slices rows.
constexpr int CHAN_RUN_SLICE = 4096;
constexpr int CHAN_SLICE_WAVES_PER_CU = 16;
struct plane_slices_t { long slices, per; };
plane_slices_t chan_plane_slices(long planes, long inner);
inline size_t chan_plane_slices_workspace_bytes(const long outer, const int C, const long inner) { return chan_planes_workspace_bytes(outer, C) * (size_t)chan_plane_slices(outer * C, inner).slices; }

// ---- which reduction: the value element (x, g) of channel c contributes ---------------------------------------------------------------------------------
struct chan_view_t { long outer; int C; long inner; };
struct RSum { __device__ float operator()(float x, float, int) const { return x; } };
struct RScaled { float s; __device__ float operator()(float x, float, int) const { return s * x; } }; // a mean (s = 1 / count), a scaled gradient sum
struct RCenteredSq { const float* mean; __device__ float operator()(float x, float, int c) const { const float w = x - mean[c]; return w * w; } };
struct RXhatG { const float* mean; const float* inv_std; __device__ float operator()(float x, float g, int c) const { return (x - mean[c]) * inv_std[c] * g; } };

// ---- kernels ---------------------------------------------------------------------------------------------------------------------------------------------
constexpr int RC_COLS = 64, RC_PHASES = 4;
// rows of C contiguous channels, `ld` elements apart.  grid (ceil(C / 64), slices); each wave owns one row phase, lanes = 64 consecutive channels.
template <class F, bool USE_G, class T>
__global__ void __launch_bounds__(256) chan_reduce_rows_kernel(F f, const T* x, const T* g, const long rows, const int C, const long ld, const long rows_per_slice, float* partial)
{
	__shared__ float red[RC_PHASES][RC_COLS];
	const int lane = threadIdx.x & 63, phase = threadIdx.x >> 6;
	const int c = blockIdx.x * RC_COLS + lane;
	const long r0 = (long)blockIdx.y * rows_per_slice;
	long r1 = r0 + rows_per_slice;
	if (r1 > rows) r1 = rows;
	float s = 0.f;
	if (c < C)
		for (long r = r0 + phase; r < r1; r += RC_PHASES) s += f((float)x[r * ld + c], USE_G ? (float)g[r * ld + c] : 0.f, c);
	red[phase][lane] = s;
	__syncthreads();
	if (phase == 0 && c < C) partial[(long)blockIdx.y * C + c] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}
// planes of `inner` contiguous elements, ONE WAVE PER PLANE (16-byte lanes when the plane allows: a workgroup per plane left 7 x 7 planes with 49 busy threads), partial[o][c].
template <class T> struct pack16 { typedef T type __attribute__((ext_vector_type(16 / sizeof(T)))); }; // one 16-byte access: 4 floats / 8 halves
template <class F, bool USE_G, class T>
__global__ void __launch_bounds__(256) chan_reduce_planes_kernel(F f, const T* x, const T* g, const int C, const long inner, const long planes, float* partial)
{
	constexpr int W = 16 / sizeof(T);
	typedef typename pack16<T>::type V;
	const int lane = threadIdx.x & 63;
	const long nw = (long)gridDim.x * 4;
	for (long pl = (long)blockIdx.x * 4 + (threadIdx.x >> 6); pl < planes; pl += nw) {
		const int c = (int)(pl % C);
		const T* const xp = x + pl * inner;
		const T* const gp = USE_G ? g + pl * inner : x;
		float s = 0.f;
		if ((inner % W) == 0 && ((((uintptr_t)xp) | ((uintptr_t)gp)) & 15) == 0) {
			const long nv = inner / W;
			for (long i = lane; i < nv; i += 64) {
				const V xv = ((const V*)xp)[i];
				V gv = xv;
				if (USE_G) gv = ((const V*)gp)[i];
#pragma unroll
				for (int e = 0; e < W; e++) s += f((float)xv[e], USE_G ? (float)gv[e] : 0.f, c);
			}
		} else
			for (long i = lane; i < inner; i += 64) s += f((float)xp[i], USE_G ? (float)gp[i] : 0.f, c);
		for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
		if (lane == 0) partial[pl] = s;
	}
}
// Short planes, CHAN_SHORT_LANES lanes each -- four planes per wave, sixteen per workgroup: a wave per plane leaves a 7 x 7 plane with 49 busy lanes, one load each,
// and six shuffle steps per plane.  A plane's lanes stride it one element at a time and meet by a butterfly inside their group; partial[o][c] as above.
constexpr int CHAN_SHORT_PLANE = 128; // planes of at most this many elements take this kernel (chan_reduce_planes_sliced)
constexpr int CHAN_SHORT_LANES = 16;
template <class F, bool USE_G, class T>
__global__ void __launch_bounds__(256) chan_reduce_short_planes_kernel(F f, const T* x, const T* g, const int C, const int inner, const long planes, float* partial)
{
	constexpr int G = CHAN_SHORT_LANES, PER_WG = 256 / G;
	const int sub = threadIdx.x & (G - 1);
	const long nw = (long)gridDim.x * PER_WG;
	for (long first = (long)blockIdx.x * PER_WG; first < planes; first += nw) { // (every lane of a wave makes the same trips: the shuffles below see all of them)
		const long pl = first + threadIdx.x / G;
		float s = 0.f;
		if (pl < planes) {
			const int c = (int)(pl % C);
			const T* const xp = x + pl * inner;
			const T* const gp = USE_G ? g + pl * inner : xp;
			for (int i = sub; i < inner; i += G) s += f((float)xp[i], USE_G ? (float)gp[i] : 0.f, c);
		}
		for (int off = G / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64); // butterfly inside the G-lane group
		if (sub == 0 && pl < planes) partial[pl] = s;
	}
}
// The same with every plane cut into `slices` slices of `per` elements (chan_plane_slices), ONE WAVE PER SLICE: partial[(o * slices + slice) * C + c].  A slice whose
// start is 16-byte aligned goes in 16-byte lanes with its last len % W elements one per lane, any other one element per lane.
template <class F, bool USE_G, class T>
__global__ void __launch_bounds__(256) chan_reduce_plane_slices_kernel(F f, const T* x, const T* g, const int C, const long inner, const long planes, const long slices, const long per, float* partial)
{
	constexpr int W = 16 / sizeof(T);
	typedef typename pack16<T>::type V;
	const int lane = threadIdx.x & 63;
	const long items = planes * slices, nw = (long)gridDim.x * 4;
	for (long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6); w < items; w += nw) {
		const long pl = w / slices, sl = w - pl * slices, o = pl / C;
		const int c = (int)(pl - o * C);
		const long begin = sl * per, len = begin + per < inner ? per : inner - begin;
		const T* const xp = x + pl * inner + begin;
		const T* const gp = USE_G ? g + pl * inner + begin : xp;
		float s = 0.f;
		long done = 0;
		if (((((uintptr_t)xp) | ((uintptr_t)gp)) & 15) == 0) {
			const long nv = len / W;
			for (long i = lane; i < nv; i += 64) {
				const V xv = ((const V*)xp)[i];
				V gv = xv;
				if (USE_G) gv = ((const V*)gp)[i];
#pragma unroll
				for (int e = 0; e < W; e++) s += f((float)xv[e], USE_G ? (float)gv[e] : 0.f, c);
			}
			done = nv * W;
		}
		for (long i = done + lane; i < len; i += 64) s += f((float)xp[i], USE_G ? (float)gp[i] : 0.f, c);
		for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
		if (lane == 0) partial[(o * slices + sl) * C + c] = s;
	}
}
// Folding per-slice (per-plane) partials into per-channel sums, fixed order, 16 channels x 16 phases per workgroup (common.h).
// out0[c] (+)= sum_i p0[i][c]  and, when p1 is given, out1[c] (+)= sum_i p1[i][c]  (blockIdx.y picks the array); halves are rounded once, at the end.
template <class TO>
__global__ void __launch_bounds__(256) chan_fold_kernel(const float* p0, const float* p1, const long slices, const int C, TO* out0, TO* out1, const int accumulate)
{
	__shared__ float red[FOLD_PH][FOLD_CH];
	const int ch = threadIdx.x & (FOLD_CH - 1), phase = threadIdx.x / FOLD_CH;
	const int c = blockIdx.x * FOLD_CH + ch;
	const float* const p = blockIdx.y ? p1 : p0;
	TO* const out = blockIdx.y ? out1 : out0;
	red[phase][ch] = c < C ? fold_slices(p, slices, C, c, phase) : 0.f;
	__syncthreads();
	if (phase == 0 && c < C) {
		const float v = fold_phases(red, ch);
		out[c] = (TO)(accumulate ? (float)out[c] + v : v);
	}
}

// Per-IMAGE column sums of a product, 16-byte lanes: partial[slice][n][c] = sum over the slice's pixels r of (p g[n][r][c]) x[n][r][c] and, DL, on the way
// d[n][r][c] = (p g[n][r][c]) s[n][c] -- g and x are read once for both.  (The rows kernel above sums ONE matrix: a launch per image would be 2 N launches.)
// grid (channel-vector tiles, pixel slices, N); a workgroup is `cvt` channel vectors (a power of two) x 256 / cvt pixel phases; the phases meet in LDS, in order.
// The slices are folded by chan_fold_kernel over N * C columns.
struct scaled_rows_plan_t { int cvt_log2, tiles; long slices, rows_per_slice; };
scaled_rows_plan_t scaled_rows_plan(int N, int cv, long P); // cv = channel vectors per pixel
template <class T, bool DL>
__global__ void __launch_bounds__(256) scaled_rows_image_kernel(const T* g, const T* x, const T* s, T* d, float* partial, const float p, const int cv, const int cvt_log2, const unsigned P, const unsigned rows_per_slice)
{
	constexpr int W = 16 / sizeof(T);
	typedef typename pack16<T>::type V;
	__shared__ float red[256 * W];
	const int cvt = 1 << cvt_log2, q = threadIdx.x & (cvt - 1), phase = threadIdx.x >> cvt_log2, phases = 256 >> cvt_log2;
	const int c = blockIdx.x * cvt + q, n = blockIdx.z, N = gridDim.z;
	const unsigned r0 = blockIdx.y * rows_per_slice, r1 = r0 + rows_per_slice < P ? r0 + rows_per_slice : P;
	float acc[W];
#pragma unroll
	for (int e = 0; e < W; e++) acc[e] = 0.f;
	if (c < cv) {
		V sv = {};
		if (DL) sv = ((const V*)s)[(size_t)n * cv + c];
		for (unsigned r = r0 + phase; r < r1; r += phases) {
			const size_t i = ((size_t)n * P + r) * cv + c;
			const V gv = ((const V*)g)[i], xv = ((const V*)x)[i];
			V o;
#pragma unroll
			for (int e = 0; e < W; e++) {
				const float pg = p * (float)gv[e];
				acc[e] += pg * (float)xv[e];
				if (DL) o[e] = (T)f32_rounded(pg * (float)sv[e]);
			}
			if (DL) ((V*)d)[i] = o;
		}
	}
#pragma unroll
	for (int e = 0; e < W; e++) red[threadIdx.x * W + e] = acc[e];
	__syncthreads();
	if (phase == 0 && c < cv) {
		float* const out = partial + ((size_t)blockIdx.y * N + n) * ((size_t)cv * W) + (size_t)c * W;
#pragma unroll
		for (int e = 0; e < W; e++) {
			float t = red[q * W + e];
			for (int ph = 1; ph < phases; ph++) t += red[((ph << cvt_log2) + q) * W + e];
			out[e] = t;
		}
	}
}
template <class T>
static void scaled_rows_image_launch(const scaled_rows_plan_t& sp, const T* g, const T* x, const T* s, T* d, float* partial, const float p, const int N, const int C, const unsigned P, hipStream_t stream)
{
	const int cv = C / (int)(16 / sizeof(T));
	const dim3 grid(sp.tiles, (unsigned)sp.slices, N);
	if (d) hipLaunchKernelGGL(HIP_KERNEL_NAME(scaled_rows_image_kernel<T, true>), grid, dim3(256), 0, stream, g, x, s, d, partial, p, cv, sp.cvt_log2, P, (unsigned)sp.rows_per_slice);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(scaled_rows_image_kernel<T, false>), grid, dim3(256), 0, stream, g, x, s, d, partial, p, cv, sp.cvt_log2, P, (unsigned)sp.rows_per_slice);
	HIP_ENFORCE(hipGetLastError());
}

// Per-IMAGE column sums of ONE tensor (the NHWC global average pool: x[n][r][c] -> out[n][c]), the same grid, workgroup shape and plan (scaled_rows_plan):
// partial[slice][n][c] = sum over the slice's rows r of f(x[n][r][c]).  W elements per lane: a 16-byte vector where the columns are whole vectors and x is
// 16-byte aligned, or 1 (cv counts lanes per row either way: C / W).  The slices are folded by chan_fold_kernel over N * C columns.
template <class F, class T, int W>
__global__ void __launch_bounds__(256) rows_image_sum_kernel(F f, const T* x, float* partial, const int cv, const int cvt_log2, const unsigned P, const unsigned rows_per_slice)
{
	typedef T V __attribute__((ext_vector_type(W)));
	__shared__ float red[256 * W];
	const int cvt = 1 << cvt_log2, q = threadIdx.x & (cvt - 1), phase = threadIdx.x >> cvt_log2, phases = 256 >> cvt_log2;
	const int c = blockIdx.x * cvt + q, n = blockIdx.z, N = gridDim.z;
	const unsigned r0 = blockIdx.y * rows_per_slice, r1 = r0 + rows_per_slice < P ? r0 + rows_per_slice : P;
	float acc[W];
#pragma unroll
	for (int e = 0; e < W; e++) acc[e] = 0.f;
	if (c < cv)
		for (unsigned r = r0 + phase; r < r1; r += phases) {
			const V xv = ((const V*)x)[((size_t)n * P + r) * cv + c];
#pragma unroll
			for (int e = 0; e < W; e++) acc[e] += f((float)xv[e], 0.f, c * W + e);
		}
#pragma unroll
	for (int e = 0; e < W; e++) red[threadIdx.x * W + e] = acc[e];
	__syncthreads();
	if (phase == 0 && c < cv) {
		float* const out = partial + ((size_t)blockIdx.y * N + n) * ((size_t)cv * W) + (size_t)c * W;
#pragma unroll
		for (int e = 0; e < W; e++) {
			float t = red[q * W + e];
			for (int ph = 1; ph < phases; ph++) t += red[((ph << cvt_log2) + q) * W + e];
			out[e] = t;
		}
	}
}
inline size_t rows_image_workspace_bytes(const int N, const int C, const int cv, const long P) { return sizeof(float) * (size_t)scaled_rows_plan(N, cv, P).slices * (size_t)N * (size_t)C; }

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------------------
// one plane per wave over the WHOLE tensor, no grid-stride cap (round 3): the same lesson as the element-wise maps (section 3.2 of DESIGN.md -- a few
// thousand workgroups striding a multi-GB tensor keep DRAM pages from all over it in flight, a front of workgroups walking it in order does not; the
// capped form ran the batch-norm passes at ~3.4 TB/s).  TUNE_GRID_WG_PER_CU > 0 restores a cap.
static inline unsigned plane_grid(const long planes)
{
	const long want = (planes + 3) / 4, per_cu = tune(TUNE_GRID_WG_PER_CU);
	const long cap = per_cu > 0 ? (long)device_cu_count() * per_cu : 0x7fffffffL;
	return (unsigned)(want < cap ? (want > 0 ? want : 1) : cap);
}
template <class TO>
static int chan_fold(const float* partial, const long slices, const int C, TO* out, const int accumulate, hipStream_t stream)
{
	hipLaunchKernelGGL(HIP_KERNEL_NAME(chan_fold_kernel<TO>), dim3((C + FOLD_CH - 1) / FOLD_CH), dim3(256), 0, stream, partial, (const float*)0, slices, C, out, (TO*)0, accumulate);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}
// out[c] (+)= sum_r f(x[r * ld + c], g[r * ld + c], c): always the scalar rows kernel (chan_sums.cpp's colsum_f32 alone picks the 16-byte one where it can)
template <class F, bool USE_G, class T, class TO>
static int chan_reduce_rows(F f, const T* x, const T* g, const long rows, const int C, const long ld, TO* out, const int accumulate, ccv_nnc_stream_context_t* ctx)
{
	const colsum_plan_t p = colsum_plan(rows, C);
	float* const partial = (float*)workspace_of(ctx, colsum_workspace_bytes(rows, C));
	if (!partial) return CCV_NNC_EXEC_OOM;
	hipStream_t stream = stream_of(ctx);
	hipLaunchKernelGGL(HIP_KERNEL_NAME(chan_reduce_rows_kernel<F, USE_G, T>), dim3(p.col_tiles, (unsigned)p.slices), dim3(256), 0, stream, f, x, g, rows, C, ld, p.rows_per_slice, partial);
	HIP_ENFORCE(hipGetLastError());
	return chan_fold(partial, p.slices, C, out, accumulate, stream);
}
// out[c] (+)= sum over (o, i) of f(.) at [(o * C + c) * inner + i]
template <class F, bool USE_G, class T, class TO>
static int chan_reduce_planes(F f, const T* x, const T* g, const chan_view_t& v, TO* out, const int accumulate, ccv_nnc_stream_context_t* ctx)
{
	float* const partial = (float*)workspace_of(ctx, chan_planes_workspace_bytes(v.outer, v.C));
	if (!partial) return CCV_NNC_EXEC_OOM;
	hipStream_t stream = stream_of(ctx);
	const long planes = v.outer * v.C;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(chan_reduce_planes_kernel<F, USE_G, T>), dim3(plane_grid(planes)), dim3(256), 0, stream, f, x, g, v.C, v.inner, planes, partial);
	HIP_ENFORCE(hipGetLastError());
	return chan_fold(partial, v.outer, v.C, out, accumulate, stream);
}
// the same by the length of a plane: up to CHAN_SHORT_PLANE elements sixteen lanes per plane, long ones cut into slices where chan_plane_slices says so, else exactly the
// launcher above (its kernel, its order)
// which of the three kernels a view takes, and its slices: the launcher below and whoever names its launch record ask here
enum { CHAN_PLANES_SHORT = 0, CHAN_PLANES_WAVE = 1, CHAN_PLANES_SLICES = 2 };
static inline int chan_planes_form(const chan_view_t& v, plane_slices_t* const ps)
{
	ps->slices = 1; ps->per = v.inner;
	if (v.inner <= CHAN_SHORT_PLANE) return CHAN_PLANES_SHORT;
	*ps = chan_plane_slices(v.outer * v.C, v.inner);
	return ps->slices <= 1 ? CHAN_PLANES_WAVE : CHAN_PLANES_SLICES;
}
static inline const char* chan_planes_kernel_name(const chan_view_t& v)
{
	plane_slices_t ps;
	const int form = chan_planes_form(v, &ps);
	return form == CHAN_PLANES_SHORT ? "chan_reduce_short_planes_kernel" : form == CHAN_PLANES_WAVE ? "chan_reduce_planes_kernel" : "chan_reduce_plane_slices_kernel";
}
template <class F, bool USE_G, class T, class TO>
static int chan_reduce_planes_sliced(F f, const T* x, const T* g, const chan_view_t& v, TO* out, const int accumulate, ccv_nnc_stream_context_t* ctx)
{
	const long planes = v.outer * v.C;
	plane_slices_t ps;
	const int form = chan_planes_form(v, &ps);
	if (form == CHAN_PLANES_SHORT) {
		float* const partial = (float*)workspace_of(ctx, chan_planes_workspace_bytes(v.outer, v.C));
		if (!partial) return CCV_NNC_EXEC_OOM;
		hipStream_t stream = stream_of(ctx);
		const long want = (planes + 256 / CHAN_SHORT_LANES - 1) / (256 / CHAN_SHORT_LANES), per_cu = tune(TUNE_GRID_WG_PER_CU);
		const long cap = per_cu > 0 ? (long)device_cu_count() * per_cu : 0x7fffffffL;
		hipLaunchKernelGGL(HIP_KERNEL_NAME(chan_reduce_short_planes_kernel<F, USE_G, T>), dim3((unsigned)(want < cap ? (want > 0 ? want : 1) : cap)), dim3(256), 0, stream, f, x, g, v.C, (int)v.inner, planes, partial);
		HIP_ENFORCE(hipGetLastError());
		return chan_fold(partial, v.outer, v.C, out, accumulate, stream);
	}
	if (form == CHAN_PLANES_WAVE) return chan_reduce_planes<F, USE_G, T, TO>(f, x, g, v, out, accumulate, ctx);
	float* const partial = (float*)workspace_of(ctx, chan_plane_slices_workspace_bytes(v.outer, v.C, v.inner));
	if (!partial) return CCV_NNC_EXEC_OOM;
	hipStream_t stream = stream_of(ctx);
	hipLaunchKernelGGL(HIP_KERNEL_NAME(chan_reduce_plane_slices_kernel<F, USE_G, T>), dim3(plane_grid(planes * ps.slices)), dim3(256), 0, stream, f, x, g, v.C, v.inner, planes, ps.slices, ps.per, partial);
	HIP_ENFORCE(hipGetLastError());
	return chan_fold(partial, v.outer * ps.slices, v.C, out, accumulate, stream);
}
// out[n][c] = sum_r f(x[n][r][c]): N images of P rows of C contiguous columns, N <= 65535
template <class F, class T, class TO>
static int rows_image_sum(F f, const T* x, const int N, const long P, const int C, TO* out, ccv_nnc_stream_context_t* ctx)
{
	constexpr int W = 16 / sizeof(T);
	const bool vec = C % W == 0 && aligned16(x);
	const int cv = vec ? C / W : C;
	const scaled_rows_plan_t sp = scaled_rows_plan(N, cv, P);
	float* const partial = (float*)workspace_of(ctx, rows_image_workspace_bytes(N, C, cv, P));
	if (!partial) return CCV_NNC_EXEC_OOM;
	hipStream_t stream = stream_of(ctx);
	const dim3 grid(sp.tiles, (unsigned)sp.slices, N);
	if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(rows_image_sum_kernel<F, T, W>), grid, dim3(256), 0, stream, f, x, partial, cv, sp.cvt_log2, (unsigned)P, (unsigned)sp.rows_per_slice);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(rows_image_sum_kernel<F, T, 1>), grid, dim3(256), 0, stream, f, x, partial, cv, sp.cvt_log2, (unsigned)P, (unsigned)sp.rows_per_slice);
	HIP_ENFORCE(hipGetLastError());
	return chan_fold(partial, sp.slices, N * C, out, 0, stream);
}
// NHWC-style views (inner == 1) are rows of C channels, everything else planes
template <class F, bool USE_G, class T = float>
static int chan_reduce(F f, const T* x, const T* g, const chan_view_t& v, float* out, ccv_nnc_stream_context_t* ctx, const int accumulate = 0)
{
	if (v.inner == 1) return chan_reduce_rows<F, USE_G, T>(f, x, g, v.outer, v.C, v.C, out, accumulate, ctx);
	return chan_reduce_planes<F, USE_G, T>(f, x, g, v, out, accumulate, ctx);
}

} // namespace nnc
