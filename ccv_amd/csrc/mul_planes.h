// MUL of a dense 4-d activation tensor by one value per (image, channel) -- the squeeze-excite scale of an MBConv block -- forward and backward.
//
// The generic route (cmd_bcast.cpp) runs this as a one-lane-per-element map with four-dimensional index arithmetic, and the small operand's gradient as a
// reduction in which one lane walks a whole plane.  Here:
//   forward   c = (p a) b in FMul's operand order: 16-byte lanes over the flat tensor.  NCHW: the scale index is derived from the element index, a vector may
//             straddle planes (7 x 7 = 49 elements are not a whole number of vectors).  NHWC: a lane owns one channel vector of one pixel and multiplies it by
//             the matching vector of the small operand.
//   backward  ONE pass over g and the large operand: d(large) = (p g) s and d(small)[n, c] = sum over the plane of (p g)(large).  NCHW: a wave per plane
//             (four planes per workgroup) up to MP_WAVE_PLANE elements, a workgroup per plane above; lanes stride the plane, the lane sums meet in a fixed
//             tree.  NHWC: chan_sums.h's scaled_rows_image_kernel (per-image column sums) and its fold.
// Plain HIP C++ over T = float / _Float16, arithmetic in fp32, each product rounded to fp32 and then once more by the store (f32_rounded, common.h).  The sums are added in an order the shape alone decides: the
// same bits on every run, no atomics.  The products are written as (p x) y, never contracted with an addition: d(large) and c carry the bits of the
// generic route's FMul.  Every launcher expects what cmd_bcast.cpp's mul_planes_plan has checked: dense tensors of one type, the large ones 16-byte
// aligned, fewer than 2^31 elements, planes of at most MUL_PLANES_MAX_PLANE elements.
#pragma once
#include "chan_sums.h"

namespace nnc {

constexpr long MUL_PLANES_MAX_PLANE = 65536;
constexpr int MP_THREADS = 256, MP_TILE = 4; // a workgroup takes one contiguous tile of 4 x 256 vectors, as the element-wise maps of cmd_ew.cpp do
constexpr unsigned MP_WAVE_PLANE = 1024;     // planes up to this many elements: one wave each

// out = first ? (p s) x : (p x) s -- `first`: the small operand is the command's first input
__device__ __forceinline__ float mul_planes_op(const float p, const float x, const float s, const int first) { return f32_rounded(first ? (p * s) * x : (p * x) * s); }

// NCHW.  nv whole vectors of the flat tensor; its last n - nv * W elements go to the first lanes of workgroup 0.
template <class T>
__global__ void __launch_bounds__(MP_THREADS) mul_planes_nchw_kernel(const T* big, const T* small, T* out, const float p, const int first, const unsigned P, const unsigned nv, const unsigned n)
{
	constexpr int W = 16 / sizeof(T);
	typedef typename pack16<T>::type V;
	const unsigned base = blockIdx.x * (MP_TILE * MP_THREADS) + threadIdx.x;
#pragma unroll
	for (int u = 0; u < MP_TILE; u++) {
		const unsigned v = base + u * MP_THREADS;
		if (v >= nv) break;
		const V x = ((const V*)big)[v];
		const unsigned e0 = v * W;
		unsigned q = e0 / P, r = e0 - q * P;
		V o;
		if (r + W <= P) { // the whole vector inside one plane
			const float s = (float)small[q];
#pragma unroll
			for (int e = 0; e < W; e++) o[e] = (T)mul_planes_op(p, (float)x[e], s, first);
		} else {
#pragma unroll
			for (int e = 0; e < W; e++) {
				o[e] = (T)mul_planes_op(p, (float)x[e], (float)small[q], first);
				if (++r == P) { r = 0; q++; }
			}
		}
		((V*)out)[v] = o;
	}
	const unsigned t = nv * W + threadIdx.x;
	if (blockIdx.x == 0 && t < n) out[t] = (T)mul_planes_op(p, (float)big[t], (float)small[t / P], first);
}

// NHWC.  grid (tiles of an image's P * cv vectors, N); cv = C / W channel vectors per pixel.
template <class T>
__global__ void __launch_bounds__(MP_THREADS) mul_planes_nhwc_kernel(const T* big, const T* small, T* out, const float p, const int first, const unsigned cv, const unsigned per_image)
{
	constexpr int W = 16 / sizeof(T);
	typedef typename pack16<T>::type V;
	const unsigned base = blockIdx.x * (MP_TILE * MP_THREADS) + threadIdx.x;
	const size_t image = (size_t)blockIdx.y * per_image;
	const V* const sp = (const V*)small + (size_t)blockIdx.y * cv;
#pragma unroll
	for (int u = 0; u < MP_TILE; u++) {
		const unsigned v = base + u * MP_THREADS;
		if (v >= per_image) break;
		const V x = ((const V*)big)[image + v];
		const V s = sp[v % cv];
		V o;
#pragma unroll
		for (int e = 0; e < W; e++) o[e] = (T)mul_planes_op(p, (float)x[e], (float)s[e], first);
		((V*)out)[image + v] = o;
	}
}

// NCHW backward: dsmall[pl] = sum_i (p g[i]) big[i] over plane pl and, DL, dbig[i] = (p g[i]) small[pl].  WAVE: four planes per workgroup, a wave each;
// else one plane per workgroup.  A plane need not start on a 16-byte boundary: its first elements up to the boundary and its last after the final whole vector
// are taken one per lane.  Each lane adds its elements in index order, the lanes meet by halving (and, across a workgroup's four waves, as (0 + 1) + (2 + 3)).
template <class T, bool DL, bool WAVE>
__global__ void __launch_bounds__(MP_THREADS) mul_planes_back_nchw_kernel(const T* g, const T* big, const T* small, T* dbig, T* dsmall, const float p, const unsigned P, const unsigned planes)
{
	constexpr unsigned W = 16 / sizeof(T);
	typedef typename pack16<T>::type V;
	__shared__ float red[4];
	const unsigned lane = WAVE ? (threadIdx.x & 63) : threadIdx.x, lanes = WAVE ? 64 : MP_THREADS;
	const unsigned pl = WAVE ? blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
	float sum = 0.f;
	if (pl < planes) {
		const size_t begin = (size_t)pl * P;
		unsigned head = (unsigned)((W - begin % W) % W);
		if (head > P) head = P;
		const unsigned nvec = (P - head) / W, tail = P - head - nvec * W;
		const float s = DL ? (float)small[pl] : 0.f;
		if (lane < head) {
			const size_t i = begin + lane;
			const float pg = p * (float)g[i];
			sum += pg * (float)big[i];
			if (DL) dbig[i] = (T)f32_rounded(pg * s);
		}
		const size_t v0 = (begin + head) / W;
		for (unsigned k = lane; k < nvec; k += lanes) {
			const V gv = ((const V*)g)[v0 + k], xv = ((const V*)big)[v0 + k];
			V o;
#pragma unroll
			for (unsigned e = 0; e < W; e++) {
				const float pg = p * (float)gv[e];
				sum += pg * (float)xv[e];
				if (DL) o[e] = (T)f32_rounded(pg * s);
			}
			if (DL) ((V*)dbig)[v0 + k] = o;
		}
		if (lane < tail) {
			const size_t i = begin + head + (size_t)nvec * W + lane;
			const float pg = p * (float)g[i];
			sum += pg * (float)big[i];
			if (DL) dbig[i] = (T)f32_rounded(pg * s);
		}
	}
	for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
	if (WAVE) {
		if (lane == 0 && pl < planes) dsmall[pl] = (T)sum;
	} else {
		if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
		__syncthreads();
		if (threadIdx.x == 0) dsmall[pl] = (T)((red[0] + red[1]) + (red[2] + red[3]));
	}
}

// ---- launchers: the geometry cmd_bcast.cpp has checked ----------------------------------------------------------------------------------------------
struct mul_planes_geom_t { int nhwc, N, C; unsigned P; }; // N * C planes of P elements (NCHW) / N images of P pixels x C channels (NHWC)

// out = (p x) s or (p s) x; `name`: the launch record (the backward command's d(large) alone is this map of g)
template <class T>
static int mul_planes_map(const char* name, const mul_planes_geom_t& m, const T* big, const T* small, T* out, const float p, const int first, ccv_nnc_stream_context_t* ctx)
{
	constexpr int W = 16 / sizeof(T);
	const size_t n = (size_t)m.N * m.C * m.P;
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	hipStream_t stream = stream_of(ctx);
	note_kernel(name);
	char prof_name[96];
	snprintf(prof_name, sizeof(prof_name), "%s|nnc::mul_planes_%s_kernel", name, m.nhwc ? "nhwc" : "nchw");
	ProfScope prof(prof_name, 2.0 * (double)n, sizeof(T) * (2.0 * (double)n + (double)m.N * m.C), m.N, m.C, (int)m.P, 1, 1, stream);
	if (m.nhwc) {
		const unsigned cv = m.C / W, per_image = m.P * cv;
		hipLaunchKernelGGL(HIP_KERNEL_NAME(mul_planes_nhwc_kernel<T>), dim3((per_image + MP_TILE * MP_THREADS - 1) / (MP_TILE * MP_THREADS), (unsigned)m.N), dim3(MP_THREADS), 0, stream, big, small, out, p, first, cv, per_image);
	} else {
		const unsigned nv = (unsigned)(n / W);
		const unsigned blocks = nv ? (nv + MP_TILE * MP_THREADS - 1) / (MP_TILE * MP_THREADS) : 1;
		hipLaunchKernelGGL(HIP_KERNEL_NAME(mul_planes_nchw_kernel<T>), dim3(blocks), dim3(MP_THREADS), 0, stream, big, small, out, p, first, m.P, nv, (unsigned)n);
	}
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

// dbig (may be null) = (p g) small, dsmall (may be null) = the plane sums of (p g) big
template <class T>
static int mul_planes_back(const mul_planes_geom_t& m, const T* g, const T* big, const T* small, T* dbig, T* dsmall, const float p, ccv_nnc_stream_context_t* ctx)
{
	if (!dsmall) return dbig ? mul_planes_map<T>("mul_planes_back", m, g, small, dbig, p, 0, ctx) : CCV_NNC_EXEC_SUCCESS;
	const size_t n = (size_t)m.N * m.C * m.P;
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	const double bytes = sizeof(T) * ((dbig ? 3.0 : 2.0) * (double)n + (dbig ? 2.0 : 1.0) * (double)m.N * m.C);
	if (m.nhwc) {
		const scaled_rows_plan_t sp = scaled_rows_plan(m.N, m.C / (int)(16 / sizeof(T)), m.P);
		float* const partial = (float*)workspace_of(ctx, sizeof(float) * (size_t)sp.slices * m.N * m.C);
		if (!partial) return CCV_NNC_EXEC_OOM;
		hipStream_t stream = stream_of(ctx);
		{
			note_kernel("mul_planes_back");
			ProfScope prof("mul_planes_back|nnc::scaled_rows_image_kernel", 3.0 * (double)n, bytes, m.N, m.C, (int)m.P, 1, (int)sp.slices, stream);
			scaled_rows_image_launch<T>(sp, g, big, small, dbig, partial, p, m.N, m.C, m.P, stream);
		}
		note_kernel("mul_planes_fold");
		ProfScope prof("mul_planes_fold|nnc::chan_fold_kernel", (double)sp.slices * m.N * m.C, sizeof(float) * (double)sp.slices * m.N * m.C, m.N, m.C, (int)sp.slices, 1, 1, stream);
		return chan_fold(partial, sp.slices, m.N * m.C, dsmall, 0, stream);
	}
	const unsigned planes = (unsigned)(m.N * m.C);
	hipStream_t stream = stream_of(ctx);
	note_kernel("mul_planes_back");
	ProfScope prof("mul_planes_back|nnc::mul_planes_back_nchw_kernel", 3.0 * (double)n, bytes, m.N, m.C, (int)m.P, 1, 1, stream);
	if (m.P <= MP_WAVE_PLANE) {
		const dim3 grid((planes + 3) / 4);
		if (dbig) hipLaunchKernelGGL(HIP_KERNEL_NAME(mul_planes_back_nchw_kernel<T, true, true>), grid, dim3(MP_THREADS), 0, stream, g, big, small, dbig, dsmall, p, m.P, planes);
		else hipLaunchKernelGGL(HIP_KERNEL_NAME(mul_planes_back_nchw_kernel<T, false, true>), grid, dim3(MP_THREADS), 0, stream, g, big, small, dbig, dsmall, p, m.P, planes);
	} else {
		if (dbig) hipLaunchKernelGGL(HIP_KERNEL_NAME(mul_planes_back_nchw_kernel<T, true, false>), dim3(planes), dim3(MP_THREADS), 0, stream, g, big, small, dbig, dsmall, p, m.P, planes);
		else hipLaunchKernelGGL(HIP_KERNEL_NAME(mul_planes_back_nchw_kernel<T, false, false>), dim3(planes), dim3(MP_THREADS), 0, stream, g, big, small, dbig, dsmall, p, m.P, planes);
	}
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

} // namespace nnc
