// Depthwise convolution (groups == channels == filters: one kh x kw stencil per channel, no contraction) on gfx950.
//   forward        b[n, y, x, c] = bias[c] + sum_{i,j} w[c][i][j] * a[n, y * s - p + i * d, x * s - p + j * d, c]
//   data gradient  h[n, y, x, c] = sum_{i,j} w[c][i][j] * g[n, (y + p - i * d) / s, (x + p - j * d) / s, c]   (where the division is exact: mfma_gemm.h conv_dgrad)
//   filter grad.   dw[c][i][j]   = sum_{n,oy,ox} g[n, oy, ox, c] * a[n, oy * s - p + i * d, ox * s - p + j * d, c],   dbias[c] = sum g
// Forward and data gradient are ONE stencil kernel per layout: the data gradient at stride 1 is the forward stencil with mirrored taps and
// padding (k - 1) * d - p (`flip`); at larger strides the source coordinate is the hole pattern above (`holes`).  Every kernel is templated over the
// element type (float, half_t) and sums in fp32.  With one input and one output channel per group the filter [K][1][kh][kw] (NCHW) and
// [K][kh][kw][1] (NHWC) are the same bytes: [C][kh * kw].
//   NHWC: a lane owns one 16-byte channel vector of one output pixel; the filter of the workgroup's channel block lies in LDS as [tap][channel].
//   NCHW: a workgroup stages whole (n, c) planes -- several small ones, or a band of rows of a large one -- into LDS as fp32 with 16-byte loads of the
//         contiguous span they occupy, then every lane computes runs of four outputs along W from it (3 x 3 / 5 x 5 at stride 1 / 2: the taps' row segment
//         in registers; anything else one output per lane).
//   Filter gradient: per-slice partial sums [slices][C][kh * kw + 1] (the + 1: the bias gradient) in the stream workspace, folded in a fixed order by
//         conv_dw_fold_kernel (common.h fold_slices / fold_phases): no atomics, the same bits every run.
#pragma once
#include "common.h"
#include "isa.h"
#include "mfma_gemm.h"

namespace nnc {

template <class T> struct DwVec;
template <> struct DwVec<float> { enum { V = 4 }; typedef floatx4 type; };
template <> struct DwVec<half_t> { enum { V = 8 }; typedef halfx8 type; };

struct DwGeom {
	int N, C;
	int SH, SW;   // the map the stencil reads (forward: the input; data gradient: the output gradient; filter gradient: the input)
	int DH, DW;   // the map it writes (filter gradient: the output gradient)
	int kh, kw, sy, sx, py, px, dy, dx;
	int holes;    // data gradient at stride > 1
	int flip;     // taps mirrored
};

constexpr int DW_MAX_K = 7;               // kh, kw
constexpr int DW_CHAN_BLOCK = 256;        // NHWC: channels of one workgroup
constexpr int DW_LDS_SRC = 8192;          // NCHW stencil: fp32 source elements a workgroup stages (32 KB: five workgroups per CU)
constexpr int DW_MAX_PLANES = 64;         // ... and the planes it takes at most (their filters: 64 * 49 floats)
constexpr int DW_RUN = 4;                 // outputs along W per lane in the register-segment form
constexpr int DW_LDS_WGRAD = 4096;        // NCHW filter gradient: fp32 elements of the input AND of the output gradient per workgroup

// source coordinate of tap t for output coordinate o, or -1
__device__ __forceinline__ int dw_src(const int o, const int t, const int s, const int p, const int d, const int S, const int holes)
{
	if (!holes) {
		const int c = o * s - p + t * d;
		return (unsigned)c < (unsigned)S ? c : -1;
	}
	const int u = o + p - t * d;
	if (u < 0) return -1;
	int c, r; // (the stride is at most 4 and wave-uniform: shifts, or a division by a constant, not the ~40 instructions of a 32-bit division per tap)
	switch (s) {
		case 1: c = u; r = 0; break;
		case 2: c = u >> 1; r = u & 1; break;
		case 3: c = (int)((unsigned)u / 3u); r = u - 3 * c; break;
		case 4: c = u >> 2; r = u & 3; break;
		default: c = u / s; r = u - c * s; break;
	}
	return r == 0 && c < S ? c : -1;
}

// ---- NHWC stencil ---------------------------------------------------------------------------------------------------------------
// grid = channel blocks x pixel blocks; thread = (pixel slot, channel vector), channel vectors fastest: a wave's loads are whole pixels' channel rows
template <class T>
static __global__ void __launch_bounds__(256) conv_dw_nhwc_kernel(const T* __restrict__ src, const T* __restrict__ w, const T* __restrict__ bias, T* __restrict__ dst, const DwGeom g, const int CV, const int cvb, const int ncb, const int pixblocks, const int pixels, const FastDiv d_w, const FastDiv d_h)
{
	constexpr int V = DwVec<T>::V;
	typedef typename DwVec<T>::type vec;
	HIP_DYNAMIC_SHARED(float, f) // [kh * kw][cvb * V]: the launcher sizes it
	const int kk = g.kh * g.kw;
	const int cb = blockIdx.x % ncb, pb = blockIdx.x / ncb;
	const int c0 = cb * cvb * V, fs = cvb * V;
	const int cbn = g.C - c0 < fs ? g.C - c0 : fs;
	for (int e = threadIdx.x; e < kk * cbn; e += 256) {
		const int cl = e / kk, t = e - cl * kk;
		f[t * fs + cl] = (float)w[(long)(c0 + cl) * kk + (g.flip ? kk - 1 - t : t)];
	}
	__syncthreads();
	const int cv = threadIdx.x % cvb, ps = threadIdx.x / cvb, PB = 256 / cvb;
	if (ps >= PB || cb * cvb + cv >= CV) return;
	const int c = c0 + cv * V;
	float b[V];
#pragma unroll
	for (int v = 0; v < V; v++) b[v] = bias ? (float)bias[c + v] : 0.f;
	for (int pix = pb * PB + ps; pix < pixels; pix += pixblocks * PB) {
		const int r = d_w.div(pix), x = pix - r * g.DW;
		const int n = d_h.div(r), y = r - n * g.DH;
		float acc[V];
#pragma unroll
		for (int v = 0; v < V; v++) acc[v] = b[v];
		for (int i = 0; i < g.kh; i++) {
			const int iy = dw_src(y, i, g.sy, g.py, g.dy, g.SH, g.holes);
			if (iy < 0) continue;
			const T* const row = src + ((long)n * g.SH + iy) * g.SW * g.C + c;
			for (int j = 0; j < g.kw; j++) {
				const int ix = dw_src(x, j, g.sx, g.px, g.dx, g.SW, g.holes);
				if (ix < 0) continue;
				const vec sv = *(const vec*)(row + (long)ix * g.C);
				const float* const ff = f + (i * g.kw + j) * fs + cv * V;
#pragma unroll
				for (int v = 0; v < V; v++) acc[v] += ff[v] * (float)sv[v];
			}
		}
		vec o;
#pragma unroll
		for (int v = 0; v < V; v++) o[v] = (T)acc[v];
		*(vec*)(dst + (long)pix * g.C + c) = o;
	}
}

// ---- NCHW stencil ---------------------------------------------------------------------------------------------------------------
// src[e0, e0 + L) -> dst[0, L) as fp32, 16-byte loads where a whole aligned vector lies inside the span (the tensor's base is 16-byte aligned)
template <class T>
__device__ __forceinline__ void dw_stage(const T* __restrict__ src, const long e0, const long L, float* __restrict__ dst)
{
	constexpr int V = DwVec<T>::V;
	typedef typename DwVec<T>::type vec;
	const long a0 = e0 & ~(long)(V - 1), e1 = e0 + L;
	for (long idx = a0 + (long)threadIdx.x * V; idx < e1; idx += 256 * V) {
		if (idx >= e0 && idx + V <= e1) {
			const vec v = *(const vec*)(src + idx);
#pragma unroll
			for (int k = 0; k < V; k++) dst[idx - e0 + k] = (float)v[k];
		} else {
			for (int k = 0; k < V; k++)
				if (idx + k >= e0 && idx + k < e1) dst[idx + k - e0] = (float)src[idx + k];
		}
	}
}

template <class T> struct DwRun;
template <> struct DwRun<float> { typedef floatx4 type; };
template <> struct DwRun<half_t> { typedef halfx4 type; };

// A workgroup = P consecutive planes (whole, when P * SH * SW fits DW_LDS_SRC) or rows [y0, y0 + TB) of one plane's output.
// K > 0: K x K taps, stride S, no dilation, no holes -- a lane computes DW_RUN outputs along W, each tap row's source segment in registers.
// K == 0: anything dw_src() describes, one output per lane.  d_x divides by the items per output row (runs, or outputs), d_t by TB.
template <class T, int K, int S>
static __global__ void __launch_bounds__(256) conv_dw_nchw_kernel(const T* __restrict__ src, const T* __restrict__ w, const T* __restrict__ bias, T* __restrict__ dst, const DwGeom g, const int planes, const int P, const int TB, const int nbands, const FastDiv d_x, const FastDiv d_t)
{
	__shared__ float xs[DW_LDS_SRC];
	HIP_DYNAMIC_SHARED(float, fs) // [P][kh * kw]: the launcher sizes it
	const int kk = g.kh * g.kw;
	const int band = blockIdx.x % nbands, plane0 = (blockIdx.x / nbands) * P;
	const int np = planes - plane0 < P ? planes - plane0 : P;
	const int y0 = band * TB;
	int r0, r1;
	if (P > 1 || nbands == 1) { r0 = 0; r1 = g.SH; }
	else if (!g.holes) { r0 = y0 * g.sy - g.py; r1 = (y0 + TB - 1) * g.sy - g.py + (g.kh - 1) * g.dy + 1; }
	else { const int lo = y0 + g.py - (g.kh - 1) * g.dy; r0 = lo > 0 ? (lo + g.sy - 1) / g.sy : 0; r1 = (y0 + TB - 1 + g.py) / g.sy + 1; }
	if (r0 < 0) r0 = 0;
	if (r1 > g.SH) r1 = g.SH;
	const long L = r1 > r0 ? ((long)(np - 1) * g.SH + (r1 - r0)) * g.SW : 0;
	if (L > DW_LDS_SRC) return; // (the launcher's plan keeps every workgroup inside: conv_dw_nchw_plan)
	if (L > 0) dw_stage<T>(src, ((long)plane0 * g.SH + r0) * g.SW, L, xs);
	for (int e = threadIdx.x; e < np * kk; e += 256) {
		const int pl = e / kk, t = e - pl * kk;
		fs[e] = (float)w[(long)((plane0 + pl) % g.C) * kk + (g.flip ? kk - 1 - t : t)];
	}
	__syncthreads();
	const int XN = d_x.d, items = np * TB * XN;
	for (int it = threadIdx.x; it < items; it += 256) {
		const int q = d_x.div(it), xr = it - q * XN;
		const int pl = d_t.div(q), y = y0 + (q - pl * TB);
		if (y >= g.DH) continue;
		const int plane = plane0 + pl;
		const float b = bias ? (float)bias[plane % g.C] : 0.f;
		const float* const fp = fs + pl * kk;
		const float* const xp = xs + ((long)pl * g.SH - r0) * g.SW; // element (iy, ix) of this plane: xp[iy * SW + ix], read only for r0 <= iy < r1
		T* const orow = dst + ((long)plane * g.DH + y) * g.DW;
		if (K > 0) {
			constexpr int SEG = (DW_RUN - 1) * S + (K > 0 ? K : 1);
			const int x0 = xr * DW_RUN;
			float acc[DW_RUN];
#pragma unroll
			for (int r = 0; r < DW_RUN; r++) acc[r] = b;
#pragma unroll
			for (int i = 0; i < K; i++) {
				const int iy = y * S - g.py + i;
				if ((unsigned)iy >= (unsigned)g.SH) continue;
				float seg[SEG];
#pragma unroll
				for (int s = 0; s < SEG; s++) {
					const int ix = x0 * S - g.px + s;
					seg[s] = (unsigned)ix < (unsigned)g.SW ? xp[iy * g.SW + ix] : 0.f;
				}
#pragma unroll
				for (int j = 0; j < K; j++) {
					const float fv = fp[i * K + j];
#pragma unroll
					for (int r = 0; r < DW_RUN; r++) acc[r] += fv * seg[r * S + j];
				}
			}
			typedef typename DwRun<T>::type run_t;
			if (x0 + DW_RUN <= g.DW && (((uintptr_t)(orow + x0)) & (sizeof(run_t) - 1)) == 0) {
				run_t o;
#pragma unroll
				for (int r = 0; r < DW_RUN; r++) o[r] = (T)acc[r];
				*(run_t*)(orow + x0) = o;
			} else {
#pragma unroll
				for (int r = 0; r < DW_RUN; r++)
					if (x0 + r < g.DW) orow[x0 + r] = (T)acc[r];
			}
		} else {
			float acc = b;
			for (int i = 0; i < g.kh; i++) {
				const int iy = dw_src(y, i, g.sy, g.py, g.dy, g.SH, g.holes);
				if (iy < 0) continue;
				for (int j = 0; j < g.kw; j++) {
					const int ix = dw_src(xr, j, g.sx, g.px, g.dx, g.SW, g.holes);
					if (ix >= 0) acc += fp[i * g.kw + j] * xp[iy * g.SW + ix];
				}
			}
			orow[xr] = (T)acc;
		}
	}
}

// ---- filter gradient + bias gradient ------------------------------------------------------------------------------------------------
// NHWC.  grid = channel blocks x row slices (rows_per output rows (n, oy) each); thread = (q, tap, channel vector): the thread sums ITS tap (tap kk: the
// bias gradient) over the pixels q, q + Q, ... of every row of the slice, for its 16-byte channel vector, and writes the partial of slice
// (row slice * Q + q) itself -- nothing meets inside the workgroup.  The taps of one pixel are neighbouring threads: g and the kh x kw window of a
// come from HBM once and from the CU's L1 after that.
template <class T>
static __global__ void __launch_bounds__(256) conv_dw_wgrad_nhwc_kernel(const T* __restrict__ gr, const T* __restrict__ a, float* __restrict__ partial, const DwGeom g, const int CV, const int cvb, const int ncb, const int Q, const int rows_per, const int rows, const FastDiv d_oh)
{
	constexpr int V = DwVec<T>::V;
	typedef typename DwVec<T>::type vec;
	const int kk = g.kh * g.kw;
	const int cb = blockIdx.x % ncb, rs = blockIdx.x / ncb;
	const int cv = threadIdx.x % cvb, r = threadIdx.x / cvb;
	const int q = r / (kk + 1), tt = r - q * (kk + 1);
	if (q >= Q || cb * cvb + cv >= CV) return;
	const int c = (cb * cvb + cv) * V;
	const int i = tt / g.kw, j = tt - i * g.kw;
	const int row0 = rs * rows_per, row1 = row0 + rows_per < rows ? row0 + rows_per : rows;
	float acc[V];
#pragma unroll
	for (int v = 0; v < V; v++) acc[v] = 0.f;
	for (int row = row0; row < row1; row++) {
		const int n = d_oh.div(row), oy = row - n * g.DH;
		int iy = 0;
		if (tt < kk) {
			iy = oy * g.sy - g.py + i * g.dy;
			if ((unsigned)iy >= (unsigned)g.SH) continue;
		}
		const T* const grow = gr + (long)row * g.DW * g.C + c;
		const T* const arow = a + ((long)n * g.SH + iy) * g.SW * g.C + c;
		for (int ox = q; ox < g.DW; ox += Q) {
			if (tt == kk) {
				const vec gv = *(const vec*)(grow + (long)ox * g.C);
#pragma unroll
				for (int v = 0; v < V; v++) acc[v] += (float)gv[v];
			} else {
				const int ix = ox * g.sx - g.px + j * g.dx;
				if ((unsigned)ix >= (unsigned)g.SW) continue;
				const vec gv = *(const vec*)(grow + (long)ox * g.C);
				const vec av = *(const vec*)(arow + (long)ix * g.C);
#pragma unroll
				for (int v = 0; v < V; v++) acc[v] += (float)gv[v] * (float)av[v];
			}
		}
	}
	float* const out = partial + ((long)(rs * Q + q) * g.C + c) * (kk + 1) + tt;
#pragma unroll
	for (int v = 0; v < V; v++) out[v * (kk + 1)] = acc[v];
}

// NCHW.  A workgroup = (block of PC channels, group of NB images, band of TB output-gradient rows): the planes (whole ones, PC * NB of them, when they fit
// DW_LDS_WGRAD; else rows of one) of a and g are staged into LDS as fp32; a group of Q neighbouring lanes (Q a power of two <= 64) owns one
// (channel, tap), each lane the columns q, q + Q, ... of every staged row of every image, and the Q sums meet by shuffles in a fixed order.
// Partial of slice (image group * nbands + band).
template <class T>
static __global__ void __launch_bounds__(256) conv_dw_wgrad_nchw_kernel(const T* __restrict__ gr, const T* __restrict__ a, float* __restrict__ partial, const DwGeom g, const int PC, const int NB, const int TB, const int nbands, const int ncb, const int Q)
{
	__shared__ float xs[DW_LDS_WGRAD];
	__shared__ float gs[DW_LDS_WGRAD];
	const int kk = g.kh * g.kw;
	int bi = blockIdx.x;
	const int band = bi % nbands; bi /= nbands;
	const int cb = bi % ncb, ng = bi / ncb;
	const int c0 = cb * PC, pc = g.C - c0 < PC ? g.C - c0 : PC;
	const int n0 = ng * NB, nb = g.N - n0 < NB ? g.N - n0 : NB;
	const int oy0 = band * TB, tb = g.DH - oy0 < TB ? g.DH - oy0 : TB;
	int r0 = 0, r1 = g.SH;
	if (nbands > 1) {
		r0 = oy0 * g.sy - g.py; r1 = (oy0 + tb - 1) * g.sy - g.py + (g.kh - 1) * g.dy + 1;
		if (r0 < 0) r0 = 0;
		if (r1 > g.SH) r1 = g.SH;
	}
	const int xrows = r1 > r0 ? r1 - r0 : 0;
	const long xl = (long)xrows * g.SW, gl = (long)tb * g.DW;                // staged elements of one plane
	const long xspan = pc > 1 ? (long)pc * g.SH * g.SW : xl, gspan = pc > 1 ? (long)pc * g.DH * g.DW : gl; // pc > 1: whole planes, contiguous over the block's channels
	if (nb * xspan > DW_LDS_WGRAD || nb * gspan > DW_LDS_WGRAD) return; // (the launcher's plan keeps every workgroup inside: conv_dw_wgrad_nchw_plan)
	for (int im = 0; im < nb; im++) {
		if (xspan > 0) dw_stage<T>(a, ((long)(n0 + im) * g.C + c0) * g.SH * g.SW + (long)r0 * g.SW, xspan, xs + im * xspan);
		dw_stage<T>(gr, ((long)(n0 + im) * g.C + c0) * g.DH * g.DW + (long)oy0 * g.DW, gspan, gs + im * gspan);
	}
	__syncthreads();
	const int U = pc * (kk + 1) * Q;
	const long slice = (long)ng * nbands + band;
	for (int u0 = 0; u0 < U; u0 += 256) { // (every lane takes every trip: the shuffles below are wave-wide)
		const int u = u0 + threadIdx.x;
		const int q = u & (Q - 1), ct = u / Q;
		const int cl = ct / (kk + 1), tt = ct - cl * (kk + 1);
		const int i = tt / g.kw, j = tt - i * g.kw;
		float acc = 0.f;
		if (u < U) {
			for (int im = 0; im < nb; im++) {
				const float* const xp = xs + im * xspan + cl * (pc > 1 ? (long)g.SH * g.SW : 0L);
				const float* const gp = gs + im * gspan + cl * (pc > 1 ? (long)g.DH * g.DW : 0L);
				for (int oy = 0; oy < tb; oy++) {
					int iy = 0;
					if (tt < kk) {
						iy = (oy0 + oy) * g.sy - g.py + i * g.dy;
						if ((unsigned)iy >= (unsigned)g.SH) continue;
						iy -= r0;
					}
					for (int ox = q; ox < g.DW; ox += Q) {
						if (tt == kk) acc += gp[oy * g.DW + ox];
						else {
							const int ix = ox * g.sx - g.px + j * g.dx;
							if ((unsigned)ix < (unsigned)g.SW) acc += gp[oy * g.DW + ox] * xp[iy * g.SW + ix];
						}
					}
				}
			}
		}
		for (int m = Q >> 1; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
		if (u < U && q == 0) partial[(slice * g.C + c0 + cl) * (kk + 1) + tt] = acc;
	}
}

// dw[c][t] (+)= sum over slices of partial[slice][c][t], dbias[c] (+)= ... [c][kk]: 16 columns x 16 phases per workgroup, fixed order (common.h)
template <class T>
static __global__ void __launch_bounds__(256) conv_dw_fold_kernel(const float* __restrict__ partial, const long slices, const int C, const int kk, T* __restrict__ dw, T* __restrict__ dbias, const int accumulate)
{
	__shared__ float red[FOLD_PH][FOLD_CH];
	const int ch = threadIdx.x & (FOLD_CH - 1), phase = threadIdx.x / FOLD_CH;
	const int cols = C * (kk + 1), col = blockIdx.x * FOLD_CH + ch;
	red[phase][ch] = col < cols ? fold_slices(partial, slices, cols, col, phase) : 0.f;
	__syncthreads();
	if (phase == 0 && col < cols) {
		const float s = fold_phases(red, ch);
		const int c = col / (kk + 1), t = col - c * (kk + 1);
		T* const o = t < kk ? (dw ? dw + (long)c * kk + t : 0) : (dbias ? dbias + c : 0);
		if (o) *o = (T)(accumulate ? (float)*o + s : s);
	}
}

} // namespace nnc
