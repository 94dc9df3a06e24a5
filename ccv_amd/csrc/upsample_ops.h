// UPSAMPLE_FORWARD / UPSAMPLE_BACKWARD (nearest, bilinear; align_corners or not) on dense CCV_16F tensors without fp32 images, NCHW and NHWC (cmd_upsample.cpp;
// tunable UPSAMPLE_HALF_NATIVE), and the geometry and coefficient functions the fp32 kernels of cmd_upsample.cpp share with them.
//
// Arithmetic: halves in and out, the fp32 kernels' expressions in between -- the same taps (nearest_src / bi_coeff: the reference's mixed float / double
// expressions), the same product order per layout, FP contraction off, every backward sum accumulated per element in (yd, xd, tap) order in fp32 -- and ONE
// rounding to half of that fp32 value (f32_rounded, common.h).  So every result is bit for bit what the fp32 kernel gives between half_up_kernel and
// half_down_kernel (the key at 0), and bit for bit half(reference(float(x))).
//
// Coefficients and hit intervals are functions of ONE axis index; the vector instances access the large tensor 16 bytes at a time:
//   interleaved (NHWC)   a lane owns W channels of one pixel (W = 8: C % 8 == 0, both bases 16-byte aligned; W = 1 otherwise): one y and one x coefficient set
//                        per W channels, taps loaded and the result stored as one vector.  Backward: the same split over source pixels, the lane walks the
//                        exact intervals of outputs that reference its pixel.
//   planar (NCHW)        forward: a lane owns W consecutive outputs of a row and keeps their x coefficients down UP_ROWS output rows; the small tensor is read by
//                        cached 2-byte loads.  W = 8 (one 16-byte store) for nearest where BW % 8 == 0 and the large base is aligned (so every row is); W = 1
//                        otherwise and for bilinear always, which measured faster that way (up_vector_width).  Backward: a lane per source element.
// The intervals: the source index of an output index is monotone along an axis, so the outputs that reference source s are the contiguous range
// [first d with key_hi(d) >= s, first d with key_lo(d) >= s + 1) -- up_first() finds a bound from an estimate and corrects it with the key function itself, so
// the range never depends on the estimate.  The loops still test every visit exactly as the fp32 kernel does: the range only bounds the walk.
// No atomics, fixed order: two runs give the same bits.  Grid-stride loops over grid_for() (GRID_WG_PER_CU); every trip derives all it uses from its own index.
// upsample_half_plan is the ONE decision: half_stage.cpp's predicate (upsample_half_applies) and the exec functions both call it.
#pragma once
#include "chan_sums.h" // half_t

namespace nnc {

enum { UPSAMPLE_NEAREST = 0, UPSAMPLE_BILINEAR = 1 };

struct UpGeom {
	int N, C, AH, AW, BH, BW;      // a = the small (source) image, b = the resampled one
	long an, ac, ah, aw;           // element strides of a for (n, c, y, x)
	long bn, bc, bh, bw;
	float rh, rw;
	int align, nchw;
};

__device__ __forceinline__ int nearest_src(const int d, const float r, const int A, const int align)
{
#pragma clang fp contract(off)
	const int s = align ? (int)((double)((float)d * r) + 0.5) : (int)(((double)d + 0.5) * (double)r);
	return s < A - 1 ? s : A - 1;
}
struct Bi { int si0, si1; float sc0, sc1; };
__device__ __forceinline__ Bi bi_coeff(const int i, const float s, const int A, const int align)
{
#pragma clang fp contract(off)
	Bi c;
	const float xs = align ? (float)i * s : (float)(((double)i + 0.5) * (double)s - 0.5);
	c.si0 = (int)xs;
	const int t = (int)(xs + 1.f);
	c.si1 = t < A - 1 ? t : A - 1;
	c.sc1 = xs - (float)c.si0;
	c.sc0 = (float)(1.0 - (double)c.sc1);
	return c;
}

// strides and ratios of dense tensors from the extents alone
static inline bool up_geom_fill(UpGeom* g, const int nchw, const int N, const int C, const int AH, const int AW, const int BH, const int BW, const int align)
{
	g->nchw = nchw; g->N = N; g->C = C; g->AH = AH; g->AW = AW; g->BH = BH; g->BW = BW;
	if (g->AH < 1 || g->AW < 1 || g->BH < 1 || g->BW < 1) return false;
	if (g->nchw) { g->aw = 1; g->ah = g->AW; g->ac = (long)g->AH * g->AW; g->an = g->ac * g->C; g->bw = 1; g->bh = g->BW; g->bc = (long)g->BH * g->BW; g->bn = g->bc * g->C; }
	else { g->ac = 1; g->aw = g->C; g->ah = (long)g->AW * g->C; g->an = g->ah * g->AH; g->bc = 1; g->bw = g->C; g->bh = (long)g->BW * g->C; g->bn = g->bh * g->BH; }
	g->align = align;
	g->rh = g->align ? (float)(g->AH - 1) / (float)(g->BH - 1 > 1 ? g->BH - 1 : 1) : (float)g->AH / (float)g->BH;
	g->rw = g->align ? (float)(g->AW - 1) / (float)(g->BW - 1 > 1 ? g->BW - 1 : 1) : (float)g->AW / (float)g->BW;
	return true;
}
// small = source-resolution tensor (forward input / backward output), big = resampled tensor
static inline bool upsample_geometry(const ccv_nnc_cmd_t& cmd, const ccv_nnc_tensor_t* small, const ccv_nnc_tensor_t* big, UpGeom* g)
{
	if (small->info.format != big->info.format) return false;
	const int nd = tensor_nd(small->info.dim);
	if (nd != tensor_nd(big->info.dim) || nd < 3 || nd > 4) return false;
	int ad[4], bd[4];
	for (int k = 0; k < 4; k++) { const int j = k - (4 - nd); ad[k] = j >= 0 ? small->info.dim[j] : 1; bd[k] = j >= 0 ? big->info.dim[j] : 1; }
	if (small->info.format == CCV_TENSOR_FORMAT_NCHW) {
		if (bd[0] != ad[0] || bd[1] != ad[1]) return false;
		return up_geom_fill(g, 1, ad[0], ad[1], ad[2], ad[3], bd[2], bd[3], cmd.info.upsample.align_corners);
	}
	if (bd[0] != ad[0] || bd[3] != ad[3]) return false;
	return up_geom_fill(g, 0, ad[0], ad[3], ad[1], ad[2], bd[1], bd[2], cmd.info.upsample.align_corners);
}

// ---- hit intervals -----------------------------------------------------------------------------------------------------------------------------------
// The source index an output index d references along an axis, as the kernels compute it.  HI = 0: nearest_src, or the bilinear lower tap si0; HI = 1: the
// bilinear upper tap si1 (>= si0).  Both are monotone in d for a ratio > 0.
template <int TYPE, int HI>
__device__ __forceinline__ int up_key(const int d, const float r, const int A, const int align)
{
	if (TYPE == UPSAMPLE_NEAREST) return nearest_src(d, r, A, align);
	const Bi c = bi_coeff(d, r, A, align);
	return HI ? c.si1 : c.si0;
}
// the first d in [0, B] with up_key(d) >= t (B: none).  The estimate t / r only sets where the walk starts.
template <int TYPE, int HI>
__device__ __forceinline__ int up_first(const int t, const float r, const int A, const int B, const int align)
{
	const float q = (float)t / r;
	int e = q >= (float)B ? B : (int)q;
	while (e > 0 && up_key<TYPE, HI>(e - 1, r, A, align) >= t) e--;
	while (e < B && up_key<TYPE, HI>(e, r, A, align) < t) e++;
	return e;
}
// outputs that can reference source s: [lo, hi] (empty: lo > hi)
template <int TYPE>
__device__ __forceinline__ void up_hits(const int s, const float r, const int A, const int B, const int align, int& lo, int& hi)
{
	lo = up_first<TYPE, TYPE == UPSAMPLE_BILINEAR ? 1 : 0>(s, r, A, B, align);
	hi = up_first<TYPE, 0>(s + 1, r, A, B, align) - 1;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------------------------
constexpr int UP_THREADS = 256;
constexpr int UP_ROWS = 4; // planar forward: the output rows a lane walks with one set of x coefficients

// interleaved forward: idx = (pixel of b) * cv + channel vector, cv = C / W
template <int TYPE, int W>
__global__ void __launch_bounds__(UP_THREADS) up_forw_nhwc_kernel(const UpGeom g, const half_t* a, half_t* b, const unsigned cv, const unsigned total)
{
#pragma clang fp contract(off) // as the fp32 kernels: the reference rounds every product and sum separately
	typedef half_t V __attribute__((ext_vector_type(W)));
	const unsigned stride = gridDim.x * blockDim.x;
	for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
		unsigned p = idx / cv;
		const unsigned cq = idx - p * cv;
		const int xd = (int)(p % (unsigned)g.BW);
		p /= (unsigned)g.BW;
		const int yd = (int)(p % (unsigned)g.BH);
		const unsigned n = p / (unsigned)g.BH;
		const V* const ap = (const V*)(a + (size_t)n * g.an) + cq;
		V o;
		if (TYPE == UPSAMPLE_NEAREST) o = ap[((size_t)nearest_src(yd, g.rh, g.AH, g.align) * g.AW + nearest_src(xd, g.rw, g.AW, g.align)) * cv];
		else {
			const Bi y = bi_coeff(yd, g.rh, g.AH, g.align), x = bi_coeff(xd, g.rw, g.AW, g.align);
			const V a00 = ap[((size_t)y.si0 * g.AW + x.si0) * cv], a01 = ap[((size_t)y.si0 * g.AW + x.si1) * cv];
			const V a10 = ap[((size_t)y.si1 * g.AW + x.si0) * cv], a11 = ap[((size_t)y.si1 * g.AW + x.si1) * cv];
			const float w00 = x.sc0 * y.sc0, w01 = x.sc1 * y.sc0, w10 = x.sc0 * y.sc1, w11 = x.sc1 * y.sc1; // NHWC pre-multiplies the weights
#pragma unroll
			for (int e = 0; e < W; e++) o[e] = (half_t)f32_rounded((float)a00[e] * w00 + (float)a01[e] * w01 + (float)a10[e] * w10 + (float)a11[e] * w11);
		}
		((V*)b)[idx] = o;
	}
}

// interleaved backward: idx = (pixel of a) * cv + channel vector
template <int TYPE, int W>
__global__ void __launch_bounds__(UP_THREADS) up_back_nhwc_kernel(const UpGeom g, const half_t* b, half_t* a, const unsigned cv, const unsigned total)
{
#pragma clang fp contract(off)
	typedef half_t V __attribute__((ext_vector_type(W)));
	const unsigned stride = gridDim.x * blockDim.x;
	for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
		unsigned p = idx / cv;
		const unsigned cq = idx - p * cv;
		const int xs = (int)(p % (unsigned)g.AW);
		p /= (unsigned)g.AW;
		const int ys = (int)(p % (unsigned)g.AH);
		const unsigned n = p / (unsigned)g.AH;
		const V* const bp = (const V*)(b + (size_t)n * g.bn) + cq;
		int ylo, yhi, xlo, xhi;
		up_hits<TYPE>(ys, g.rh, g.AH, g.BH, g.align, ylo, yhi);
		up_hits<TYPE>(xs, g.rw, g.AW, g.BW, g.align, xlo, xhi);
		float sum[W];
#pragma unroll
		for (int e = 0; e < W; e++) sum[e] = 0.f;
		for (int yd = ylo; yd <= yhi; yd++) {
			if (TYPE == UPSAMPLE_NEAREST) {
				if (nearest_src(yd, g.rh, g.AH, g.align) != ys) continue;
				for (int xd = xlo; xd <= xhi; xd++) {
					if (nearest_src(xd, g.rw, g.AW, g.align) != xs) continue;
					const V gv = bp[((size_t)yd * g.BW + xd) * cv];
#pragma unroll
					for (int e = 0; e < W; e++) sum[e] += (float)gv[e];
				}
			} else {
				const Bi y = bi_coeff(yd, g.rh, g.AH, g.align);
				const bool y0 = y.si0 == ys, y1 = y.si1 == ys;
				if (!y0 && !y1) continue;
				for (int xd = xlo; xd <= xhi; xd++) {
					const Bi x = bi_coeff(xd, g.rw, g.AW, g.align);
					const bool x0 = x.si0 == xs, x1 = x.si1 == xs;
					if (!x0 && !x1) continue;
					const V gv = bp[((size_t)yd * g.BW + xd) * cv];
					const float w00 = x.sc0 * y.sc0, w01 = x.sc1 * y.sc0, w10 = x.sc0 * y.sc1, w11 = x.sc1 * y.sc1;
					// tap order of the reference's scatter: (y0,x0) (y0,x1) (y1,x0) (y1,x1), g * (sc_x * sc_y)
#pragma unroll
					for (int e = 0; e < W; e++) {
						const float gf = (float)gv[e];
						if (y0 && x0) sum[e] += gf * w00;
						if (y0 && x1) sum[e] += gf * w01;
						if (y1 && x0) sum[e] += gf * w10;
						if (y1 && x1) sum[e] += gf * w11;
					}
				}
			}
		}
		V o;
#pragma unroll
		for (int e = 0; e < W; e++) o[e] = (half_t)f32_rounded(sum[e]);
		((V*)a)[idx] = o;
	}
}

// planar forward: idx = ((plane * chunks) + chunk of UP_ROWS output rows) * xgroups + group of W output columns; neighbouring lanes hold neighbouring column
// groups of one row, and a lane keeps its column group's x coefficients for its UP_ROWS rows
template <int TYPE, int W>
__global__ void __launch_bounds__(UP_THREADS) up_forw_nchw_kernel(const UpGeom g, const half_t* a, half_t* b, const unsigned xgroups, const unsigned chunks, const unsigned total)
{
#pragma clang fp contract(off)
	typedef half_t V __attribute__((ext_vector_type(W)));
	const unsigned stride = gridDim.x * blockDim.x;
	for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
		unsigned p = idx / xgroups;
		const int x0 = (int)(idx - p * xgroups) * W;
		const int y0 = (int)(p % chunks) * UP_ROWS;
		p /= chunks;
		const half_t* const ap = a + (size_t)p * g.ac;
		half_t* const bp = b + (size_t)p * g.bc;
		int sx[W];
		Bi x[W];
#pragma unroll
		for (int e = 0; e < W; e++) { // (W = 8: BW % 8 == 0, every column is inside the row)
			if (TYPE == UPSAMPLE_NEAREST) sx[e] = nearest_src(x0 + e, g.rw, g.AW, g.align);
			else x[e] = bi_coeff(x0 + e, g.rw, g.AW, g.align);
		}
#pragma unroll
		for (int r = 0; r < UP_ROWS; r++) {
			const int yd = y0 + r;
			if (yd >= g.BH) break;
			V o;
			if (TYPE == UPSAMPLE_NEAREST) {
				const half_t* const row = ap + (size_t)nearest_src(yd, g.rh, g.AH, g.align) * g.AW;
#pragma unroll
				for (int e = 0; e < W; e++) o[e] = row[sx[e]];
			} else {
				const Bi y = bi_coeff(yd, g.rh, g.AH, g.align);
				const half_t* const r0 = ap + (size_t)y.si0 * g.AW;
				const half_t* const r1 = ap + (size_t)y.si1 * g.AW;
#pragma unroll
				for (int e = 0; e < W; e++) {
					const float a00 = (float)r0[x[e].si0], a01 = (float)r0[x[e].si1], a10 = (float)r1[x[e].si0], a11 = (float)r1[x[e].si1];
					// NCHW multiplies tap * sc_x * sc_y
					o[e] = (half_t)f32_rounded(a00 * x[e].sc0 * y.sc0 + a01 * x[e].sc1 * y.sc0 + a10 * x[e].sc0 * y.sc1 + a11 * x[e].sc1 * y.sc1);
				}
			}
			*(V*)(bp + (size_t)yd * g.BW + x0) = o;
		}
	}
}

// planar backward: idx = (plane * AH + source row) * AW + source column, a lane per source element: neighbouring lanes read neighbouring spans of a gradient row.
// (Eight source elements per lane with a 16-byte store were measured too: slower on every row but the largest nearest one, by up to 2.2x -- second table of
// profiles/upsample_half_bench.md.)
template <int TYPE>
__global__ void __launch_bounds__(UP_THREADS) up_back_nchw_kernel(const UpGeom g, const half_t* b, half_t* a, const unsigned total)
{
#pragma clang fp contract(off)
	const unsigned stride = gridDim.x * blockDim.x;
	for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
		unsigned p = idx / (unsigned)g.AW;
		const int xs = (int)(idx - p * (unsigned)g.AW);
		const int ys = (int)(p % (unsigned)g.AH);
		p /= (unsigned)g.AH;
		const half_t* const bp = b + (size_t)p * g.bc;
		int ylo, yhi, xlo, xhi;
		up_hits<TYPE>(ys, g.rh, g.AH, g.BH, g.align, ylo, yhi);
		up_hits<TYPE>(xs, g.rw, g.AW, g.BW, g.align, xlo, xhi);
		float sum = 0.f;
		for (int yd = ylo; yd <= yhi; yd++) {
			const half_t* const row = bp + (size_t)yd * g.BW;
			if (TYPE == UPSAMPLE_NEAREST) {
				if (nearest_src(yd, g.rh, g.AH, g.align) != ys) continue;
				for (int xd = xlo; xd <= xhi; xd++)
					if (nearest_src(xd, g.rw, g.AW, g.align) == xs) sum += (float)row[xd];
			} else {
				const Bi y = bi_coeff(yd, g.rh, g.AH, g.align);
				const bool y0 = y.si0 == ys, y1 = y.si1 == ys;
				if (!y0 && !y1) continue;
				for (int xd = xlo; xd <= xhi; xd++) {
					const Bi x = bi_coeff(xd, g.rw, g.AW, g.align);
					const bool x0 = x.si0 == xs, x1 = x.si1 == xs;
					if (!x0 && !x1) continue;
					const float gv = (float)row[xd];
					// tap order of the reference's scatter: (y0,x0) (y0,x1) (y1,x0) (y1,x1), g * sc_y * sc_x
					if (y0 && x0) sum += gv * y.sc0 * x.sc0;
					if (y0 && x1) sum += gv * y.sc0 * x.sc1;
					if (y1 && x0) sum += gv * y.sc1 * x.sc0;
					if (y1 && x1) sum += gv * y.sc1 * x.sc1;
				}
			}
		}
		a[idx] = (half_t)f32_rounded(sum);
	}
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------------------------
struct upsample_plan_t { UpGeom g; int type; const half_t* small; const half_t* big; };
constexpr double UP_MAX_ELEMENTS = 2147483648.0; // the kernels index work items and pixels with 32-bit unsigned values: tensors of 2^31 elements and more are refused

// what of the decision is arithmetic on the extents: type 0 or 1, an enlargement, no zero ratio (align_corners with a source extent of 1: the command keeps
// today's route and result), fewer than 2^31 elements in either tensor
static inline bool up_geom_native(const UpGeom& g, const int type)
{
	if (type != UPSAMPLE_NEAREST && type != UPSAMPLE_BILINEAR) return false;
	if (!(g.rh <= 1.f && g.rw <= 1.f) || !(g.rh > 0.f && g.rw > 0.f)) return false;
	const double planes = (double)g.N * (double)g.C;
	return planes * (double)g.AH * (double)g.AW < UP_MAX_ELEMENTS && planes * (double)g.BH * (double)g.BW < UP_MAX_ELEMENTS;
}
static inline bool up_half_dense(const ccv_nnc_tensor_t* t) { return t && !CCV_IS_TENSOR_VIEW(t) && CCV_GET_DATA_TYPE(t->info.datatype) == CCV_16F && t->data.u8; }
// true: the key is on, nothing is accumulated, both tensors are dense CCV_16F tensors with memory of their own, and the geometry is one the kernels take -- *o
// then holds it.  false: the command keeps today's route (and today's return value).
static bool upsample_half_plan(const ccv_nnc_cmd_t cmd, const int flags, const ccv_nnc_tensor_t* small, const ccv_nnc_tensor_t* big, upsample_plan_t* const o)
{
	if (!tune(TUNE_UPSAMPLE_HALF_NATIVE) || (flags & CCV_NNC_ACCUMULATE_OUTPUT)) return false;
	if (!up_half_dense(small) || !up_half_dense(big) || small->data.u8 == big->data.u8) return false;
	if (!upsample_geometry(cmd, small, big, &o->g)) return false;
	o->type = cmd.info.upsample.type;
	o->small = (const half_t*)small->data.u8;
	o->big = (const half_t*)big->data.u8;
	return up_geom_native(o->g, o->type);
}
// W of the instance a plan runs on: 8 (16-byte accesses to the tensor the lanes are laid over) or 1.  The planar kernels are bound by their coefficient
// arithmetic and 2-byte gathers, not by their stores: bilinear forward and both backward kernels were faster a lane per element (more lanes, shorter chains,
// neighbouring lanes on neighbouring taps), so only the planar nearest forward -- a row copy with repeats -- has a vector instance.
static inline int up_vector_width(const upsample_plan_t& p, const bool forward)
{
	const UpGeom& g = p.g;
	if (tune(TUNE_UPSAMPLE_HALF_NATIVE) == 2) return 1; // (measurements: the scalar instances everywhere)
	if (!g.nchw) return g.C % 8 == 0 && aligned16(p.small) && aligned16(p.big) ? 8 : 1;
	return forward && p.type == UPSAMPLE_NEAREST && g.BW % 8 == 0 && aligned16(p.big) ? 8 : 1;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------------------
// the launch record: "upsample_forw|nnc::<kernel><type,W>" / "upsample_back|..." (ProfScope copies it; note_kernel keeps the pointer it is given, so it gets literals)
struct up_prof_name_t {
	char s[96];
	up_prof_name_t(const bool forward, const char* kernel, const int type, const int W) { snprintf(s, sizeof(s), "upsample_%s|nnc::%s<%s,%d>", forward ? "forw" : "back", kernel, type == UPSAMPLE_NEAREST ? "nearest" : "bilinear", W); }
};
template <int TYPE, int W>
static void up_launch_nhwc(const upsample_plan_t& p, const bool forward, const int blocks, const unsigned cv, const unsigned total, hipStream_t stream)
{
	if (forward) hipLaunchKernelGGL(HIP_KERNEL_NAME(up_forw_nhwc_kernel<TYPE, W>), dim3(blocks), dim3(UP_THREADS), 0, stream, p.g, p.small, (half_t*)p.big, cv, total);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(up_back_nhwc_kernel<TYPE, W>), dim3(blocks), dim3(UP_THREADS), 0, stream, p.g, p.big, (half_t*)p.small, cv, total);
}
template <int TYPE>
static void up_launch_nchw(const upsample_plan_t& p, const bool forward, const int W, const int blocks, const unsigned xgroups, const unsigned chunks, const unsigned total, hipStream_t stream)
{
	if (!forward) hipLaunchKernelGGL(HIP_KERNEL_NAME(up_back_nchw_kernel<TYPE>), dim3(blocks), dim3(UP_THREADS), 0, stream, p.g, p.big, (half_t*)p.small, total);
	else if (TYPE == UPSAMPLE_NEAREST && W == 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(up_forw_nchw_kernel<UPSAMPLE_NEAREST, 8>), dim3(blocks), dim3(UP_THREADS), 0, stream, p.g, p.small, (half_t*)p.big, xgroups, chunks, total);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(up_forw_nchw_kernel<TYPE, 1>), dim3(blocks), dim3(UP_THREADS), 0, stream, p.g, p.small, (half_t*)p.big, xgroups, chunks, total);
}
static int upsample_half_run(const upsample_plan_t& p, const bool forward, ccv_nnc_stream_context_t* ctx)
{
	const UpGeom& g = p.g;
	const int W = up_vector_width(p, forward);
	const double planes = (double)g.N * g.C, na = planes * g.AH * g.AW, nb = planes * g.BH * g.BW;
	// work items: no more than the elements of the tensor they are laid over (< 2^31)
	unsigned groups, chunks = 1, total;
	if (!g.nchw) { groups = (unsigned)(g.C / W); total = (unsigned)g.N * (unsigned)(forward ? g.BH * g.BW : g.AH * g.AW) * groups; }
	else if (forward) { groups = (unsigned)((g.BW + W - 1) / W); chunks = (unsigned)((g.BH + UP_ROWS - 1) / UP_ROWS); total = (unsigned)g.N * g.C * chunks * groups; }
	else { groups = (unsigned)g.AW; total = (unsigned)na; }
	hipStream_t stream = stream_of(ctx);
	const char* const kernel = g.nchw ? (forward ? "up_forw_nchw_kernel" : "up_back_nchw_kernel") : (forward ? "up_forw_nhwc_kernel" : "up_back_nhwc_kernel");
	const up_prof_name_t name(forward, kernel, p.type, W);
	note_kernel(g.nchw ? (forward ? "up_forw_nchw" : "up_back_nchw") : (forward ? "up_forw_nhwc" : "up_back_nhwc"));
	ProfScope prof(name.s, forward ? nb : na, sizeof(half_t) * (na + nb), g.N, g.C, g.BH, g.BW, 1, stream);
	const int blocks = grid_for(total, UP_THREADS);
	if (g.nchw) { if (p.type == UPSAMPLE_NEAREST) up_launch_nchw<UPSAMPLE_NEAREST>(p, forward, W, blocks, groups, chunks, total, stream); else up_launch_nchw<UPSAMPLE_BILINEAR>(p, forward, W, blocks, groups, chunks, total, stream); }
	else if (p.type == UPSAMPLE_NEAREST) { if (W == 8) up_launch_nhwc<UPSAMPLE_NEAREST, 8>(p, forward, blocks, groups, total, stream); else up_launch_nhwc<UPSAMPLE_NEAREST, 1>(p, forward, blocks, groups, total, stream); }
	else { if (W == 8) up_launch_nhwc<UPSAMPLE_BILINEAR, 8>(p, forward, blocks, groups, total, stream); else up_launch_nhwc<UPSAMPLE_BILINEAR, 1>(p, forward, blocks, groups, total, stream); }
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

} // namespace nnc
