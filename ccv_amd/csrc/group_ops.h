// Group-norm kernels: GROUP_NORM forward and backward over dense maps of element type T = _Float16 (a, b, g, h) with per-channel parameters and per-statistic
// statistics of type P, _Float16 ("hh") or float ("hf") (scale, bias, saved_mean, saved_inv_std, dscale, dbias).  Registered in half_stage.cpp g_native_half,
// tunable GNORM_HALF_NATIVE; the fp32 commands keep gnorm_*_kernel of cmd_groupnorm.cpp and their bits.  Semantics and the epsilon quirk: cmd_groupnorm.cpp:1-11.
//
// Two layouts (cmd_groupnorm.cpp classifies a command with geometry()):
//   planar  a statistic owns ONE contiguous run of n elements ([outer][C][inner] with the groups on C: NCHW, [N, C] maps); the parameter of an element is
//           (offset / inner) % C
//   inter   NHWC: statistic (image, group) owns H W rows of cg = C / G contiguous channels, one row every C elements; parameters per channel
// Arithmetic as in row_ops.h: fp32 throughout, operands widened on load, ONE rounding to half where a value is stored (f32_rounded), contraction written out
// (the pragma turns it off, every fma is spelled), no atomics, no per-launch host counter: the same bits on every run, and inside a captured graph.
// Statistics are centred: a planar slice lives in registers (mean, then the squares of the centred values); an interleaved lane keeps Welford's
// (count, mean, M2) of its channels; partials meet in a fixed order by Chan's formula taken over all of them at once (fold_stats).  E[x^2] - mean^2 is never formed.
//
// Two forms, chosen by shape alone:
// The reg form, planar with n <= GN_REG_MAX: one workgroup per statistic, ONE launch, the run read once and held in registers -- forward (mean, centred
// variance, b, the two statistics) and the backward command that asks for h alone.
// The split form, every other shape (slice_plan below; partials in the stream workspace):
//   forward   1. stats   a workgroup takes a slice of a statistic's run (planar) or a slice of an image's pixel rows over all C channels (inter: a lane's
//                        channels are fixed for the slice, per-channel partials are folded into per-group ones in LDS, channel by channel -- a 16-byte vector that
//                        straddles two groups is no special case) and writes (count, mean, M2) per (statistic, slice)
//             2. apply   every workgroup folds the partials of its statistic(s) in slice order and normalises its own slice; the workgroups of slice 0 store
//                        saved_mean and saved_inv_std.  a is read twice, b written once.
//   backward  with A = sum g and B = sum ah g per (image, channel), ah = (a - mean) inv_std from the STORED statistics:
//             1. sums    A and B per (image, slice, channel): g and a read once
//             2. fold    over the slices and a group's channels (s1 = inv_std sum scale A, s2 = inv_std sum scale B, left in the workspace), and over the
//                        slices and images (dbias = sum A, dscale = sum B, rounded once to their own type; skipped when no parameter gradient is asked for)
//             3. apply   h = gss - (s1 + ah s2) / n, gss = g scale inv_std; skipped when h is absent.  g and a are read twice at most.
// A lane reads all it needs of an element before it writes it: b = a and h = g are fine.
// Bases that are not 16-byte aligned, a planar run (for the backward sums: a plane) that is no multiple of 8 elements, or C no multiple of 8 (inter) take the
// scalar instance of the same kernel (row_ops.h:58-60 on why that is an instance and not a flag).
#pragma once
#include "row_ops.h"

namespace nnc {
namespace gnorm {

using optim::raw8;
using rows::lane_t;
using rows::row_reduce;
typedef _Float16 half_t;

constexpr int GN_THREADS = 256;
constexpr int GN_LANE = 8; // elements of one vector access
constexpr int GN_REG_MAX = 16384; // longest planar run of the reg form: 256 lanes x 8 vectors (tests/test_gnorm_half.py reads this line)
constexpr int GN_SLICE_MAX = 8192; // most elements of a planar slice: 256 lanes x 4 vectors, the slice in registers (tests/test_gnorm_half.py reads this line)
constexpr int GN_SLICE_MIN = 2048; // fewest elements a slice is cut down to (tests/test_gnorm_half.py reads this line)
constexpr int GN_INTER_SLICE_MIN = 8192; // inter: fewest elements (pixel rows x C) a slice is cut down to (tests/test_gnorm_half.py reads this line)
constexpr int GN_TARGET_WGS = 1024; // workgroups a launch aims at: four per CU (tests/test_gnorm_half.py reads this line)
constexpr int GN_MAX_C = 4096; // inter: channels whose per-phase partials fit the LDS of one workgroup
constexpr int GN_MAX_G = 1024; // inter: groups whose statistics fit the LDS of one workgroup
constexpr int GN_NV = GN_SLICE_MAX / (GN_THREADS * GN_LANE);
static_assert(GN_REG_MAX == GN_THREADS * 8 * GN_LANE && GN_NV == 4 && GN_SLICE_MIN % GN_LANE == 0 && GN_SLICE_MAX % GN_LANE == 0 && GN_MAX_C >= GN_THREADS * GN_LANE, "a lane holds four vectors; phases x channels <= GN_MAX_C");

// ---- the shape of a command and its slice plan ---------------------------------------------------------------------------------------------------------------
// planar: R = outer * G runs of n = cg * inner elements.  inter: outer images of `inner` pixel rows of C channels, n = cg * inner.
struct shape_t { int inter, outer, C, G, cg, inner, n, R; };
// `units` runs of `len` items each cut into slices of `per` items (a multiple of `quantum`, at least min_per, at most max_per when that is not 0): about
// GN_TARGET_WGS workgroups in all, no empty slice
struct slice_plan_t { int slices, per; };
static inline slice_plan_t slice_plan(const long units, const int len, const int quantum, const int min_per, const int max_per)
{
	long want = (GN_TARGET_WGS + units - 1) / (units > 0 ? units : 1);
	if (want < 1) want = 1;
	long per = (len + want - 1) / want;
	if (per < min_per) per = min_per;
	per = (per + quantum - 1) / quantum * quantum;
	if (max_per && per > max_per) per = max_per;
	slice_plan_t p;
	p.per = (int)per;
	p.slices = (int)((len + per - 1) / per);
	if (p.slices < 1) p.slices = 1;
	return p;
}
// forward, and the backward apply pass: slices of a run (planar, elements) or of an image's pixel rows (inter, rows)
static inline slice_plan_t map_plan(const shape_t& s)
{
	if (s.inter) return slice_plan(s.outer, s.inner, 1, (GN_INTER_SLICE_MIN + s.C - 1) / s.C, 0);
	return slice_plan(s.R, s.n, GN_LANE, GN_SLICE_MIN, GN_SLICE_MAX);
}
// the backward sums: inter as above; planar: a wave per slice of a plane (four per workgroup)
static inline slice_plan_t sums_plan(const shape_t& s)
{
	if (s.inter) return map_plan(s);
	return slice_plan(((long)s.outer * s.C + 3) / 4, s.inner, GN_LANE, GN_SLICE_MIN, 0);
}
static inline size_t fwd_workspace_bytes(const shape_t& s) { return sizeof(float) * 3 * (size_t)s.R * (size_t)map_plan(s).slices; } // [R][slices](count, mean, M2)
static inline size_t bwd_sums_floats(const shape_t& s) { return (size_t)s.outer * (size_t)sums_plan(s).slices * (size_t)s.C; } // one of [outer][slices][C]
static inline size_t bwd_workspace_bytes(const shape_t& s) { return sizeof(float) * 2 * (bwd_sums_floats(s) + (size_t)s.R); } // A, B, then [R](s1, s2)

struct args_t {
	const void *a, *g, *scale, *bias, *mean_in, *inv_std_in; // backward reads the statistics, forward writes them
	void *out, *mean, *inv_std, *dscale, *dbias; // out: b or h
	float *part, *s12; // forward: [R][slices][3]; backward: A = part, B = part + sums_floats; s12 = [R][2]
	int outer, C, G, cg, inner, n, R;
	int slices, per, sum_slices, sum_per; // of the map passes / of the backward sums
	int cvt_log2, inner8, stat_wgs; // inter: channel-vector columns of a workgroup; planar: inner % 8 == 0; fold: workgroups [0, stat_wgs) fold groups
	size_t sums_floats;
	float inv_n, epsilon;
};

// Partials (count, mean, M2) meet in two passes, each a chain of fused multiply-adds in a fixed order and without a division per partial: the pooled mean
// sum(count mean) / sum(count), then M2 = sum(M2_i + count_i (mean_i - mean)^2) -- Chan's formula for all partials at once, centred on the pooled mean.
// the statistics of run / statistic s from its partials, in slice order
__device__ __forceinline__ void fold_stats(const args_t& p, const int s, float* const mean, float* const inv_std)
{
#pragma clang fp contract(off)
	const float* const q = p.part + (size_t)s * p.slices * 3;
	float cn = 0.f, sm = 0.f, m2 = 0.f;
	for (int i = 0; i < p.slices; i++) { cn += q[3 * i]; sm = __builtin_fmaf(q[3 * i], q[3 * i + 1], sm); }
	const float m = sm / cn;
	for (int i = 0; i < p.slices; i++) { const float d = q[3 * i + 1] - m; m2 += __builtin_fmaf(q[3 * i] * d, d, q[3 * i + 2]); }
	*mean = m;
	*inv_std = 1.f / sqrtf(__builtin_fmaf(m2, p.inv_n, p.epsilon));
}
// the channel of column `col` of the run at offset `off`; `whole`: a vector lies in one channel -- one division for its eight elements
__device__ __forceinline__ unsigned channel_of(const size_t off, const int col, const bool whole, const unsigned inner, const unsigned C)
{
	return (unsigned)((off + (size_t)(whole ? col & ~(GN_LANE - 1) : col)) / inner) % C;
}

// ---- planar ------------------------------------------------------------------------------------------------------------------------------------------------------
// grid R x slices: the slice in registers, the mean, then the centred squares
template <class T, bool VEC>
__global__ void __launch_bounds__(GN_THREADS) planar_stats_kernel(const args_t p)
{
#pragma clang fp contract(off)
	typedef lane_t<GN_NV, true, VEC> L;
	__shared__ float red[rows::RED_FLOATS];
	const int s = blockIdx.x / p.slices, sl = blockIdx.x % p.slices, k0 = sl * p.per;
	const int len = p.n - k0 < p.per ? p.n - k0 : p.per;
	const L ln = { (int)threadIdx.x, len };
	float x[L::E];
	ln.load(x, (const T*)p.a + (size_t)s * p.n + k0, 0.f);
	float t[1] = { 0.f };
#pragma unroll
	for (int k = 0; k < L::E; k++) t[0] += x[k];
	row_reduce<true, false, 1>(t, red);
	const float mean = t[0] / (float)len;
	float v[1] = { 0.f };
#pragma unroll
	for (int k = 0; k < L::E; k++) {
		const float w = ln.has(k) ? x[k] - mean : 0.f;
		v[0] = __builtin_fmaf(w, w, v[0]);
	}
	row_reduce<true, false, 1>(v, red + 8);
	if (threadIdx.x == 0) {
		float* const q = p.part + ((size_t)s * p.slices + sl) * 3;
		q[0] = (float)len; q[1] = mean; q[2] = v[0];
	}
}
// grid R x slices: forward b = (a - mean) inv_std scale + bias from the folded partials; BWD h = gss - (s1 + ah s2) / n from the stored statistics
template <class T, class P, bool VEC, bool BWD>
__global__ void __launch_bounds__(GN_THREADS) planar_apply_kernel(const args_t p)
{
#pragma clang fp contract(off)
	typedef lane_t<GN_NV, true, VEC> L;
	const int s = blockIdx.x / p.slices, sl = blockIdx.x % p.slices, k0 = sl * p.per;
	const int len = p.n - k0 < p.per ? p.n - k0 : p.per;
	const L ln = { (int)threadIdx.x, len };
	const size_t off = (size_t)s * p.n + k0;
	float mean, inv_std, s1 = 0.f, s2 = 0.f;
	if constexpr (BWD) {
		mean = (float)((const P*)p.mean_in)[s]; inv_std = (float)((const P*)p.inv_std_in)[s];
		s1 = p.s12[2 * (size_t)s]; s2 = p.s12[2 * (size_t)s + 1];
	} else {
		fold_stats(p, s, &mean, &inv_std);
		if (sl == 0 && threadIdx.x == 0) {
			((P*)p.mean)[s] = (P)f32_rounded(mean);
			((P*)p.inv_std)[s] = (P)f32_rounded(inv_std);
		}
	}
	float x[L::E], g[BWD ? L::E : 1];
	ln.load(x, (const T*)p.a + off, 0.f);
	if constexpr (BWD) ln.load(g, (const T*)p.g + off, 0.f);
	const P* const scale = (const P*)p.scale;
	const P* const bias = (const P*)p.bias;
	const unsigned inner = (unsigned)p.inner, C = (unsigned)p.C;
	const bool whole = VEC && p.inner8; // a vector lies in one channel: one division for its eight elements
#pragma unroll
	for (int k = 0; k < L::E; k++) {
		const int col = ln.col(k);
		unsigned ch = 0;
		if ((scale || bias) && col < len) ch = channel_of(off, col, whole, inner, C);
		const float ah = (x[k] - mean) * inv_std;
		if constexpr (BWD) {
			float gs = g[k];
			if (scale) gs = gs * (float)scale[ch];
			gs = gs * inv_std;
			x[k] = __builtin_fmaf(-p.inv_n, __builtin_fmaf(ah, s2, s1), gs);
		} else {
			float y = ah;
			if (scale) y = y * (float)scale[ch];
			if (bias) y = y + (float)bias[ch];
			x[k] = y;
		}
	}
	ln.store((T*)p.out + off, x);
}
// backward sums, a wave per (plane, slice): A = sum g, B = sum ah g -> [outer][sum_slices][C]
template <class T, class P, bool VEC>
__global__ void __launch_bounds__(GN_THREADS) planar_sums_kernel(const args_t p)
{
#pragma clang fp contract(off)
	const long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (u >= (long)p.outer * p.C * p.sum_slices) return; // (a whole wave: no barrier follows)
	const int lane = threadIdx.x & 63;
	const int plane = (int)(u / p.sum_slices), sl = (int)(u % p.sum_slices);
	const int o = plane / p.C, c = plane % p.C, s = o * p.G + c / p.cg;
	const float mean = (float)((const P*)p.mean_in)[s], inv_std = (float)((const P*)p.inv_std_in)[s];
	const int k0 = sl * p.sum_per, k1 = k0 + p.sum_per < p.inner ? k0 + p.sum_per : p.inner;
	const T* const ap = (const T*)p.a + (size_t)plane * p.inner;
	const T* const gp = (const T*)p.g + (size_t)plane * p.inner;
	float v[2] = { 0.f, 0.f };
	if constexpr (VEC) {
		for (int i = k0 + lane * GN_LANE; i < k1; i += 64 * GN_LANE) {
			raw8<T> ra, rg;
			ra.load(ap + i); rg.load(gp + i);
#pragma unroll
			for (int e = 0; e < GN_LANE; e++) {
				const float gg = rg.get(e);
				v[0] += gg;
				v[1] = __builtin_fmaf((ra.get(e) - mean) * inv_std, gg, v[1]);
			}
		}
	} else {
		for (int i = k0 + lane; i < k1; i += 64) {
			const float gg = (float)gp[i];
			v[0] += gg;
			v[1] = __builtin_fmaf(((float)ap[i] - mean) * inv_std, gg, v[1]);
		}
	}
	row_reduce<false, false, 2>(v, (float*)0);
	if (lane == 0) {
		const size_t q = ((size_t)o * p.sum_slices + sl) * p.C + c;
		p.part[q] = v[0];
		p.part[p.sums_floats + q] = v[1];
	}
}

// ---- planar, the reg form: n <= GN_REG_MAX, one workgroup per statistic, ONE launch; the run is read once and lives in registers ---------------------------------
template <class T, class P, int NV, bool VEC>
__global__ void __launch_bounds__(GN_THREADS) planar_reg_fwd_kernel(const args_t p)
{
#pragma clang fp contract(off)
	typedef lane_t<NV, true, VEC> L;
	__shared__ float red[rows::RED_FLOATS];
	const int s = blockIdx.x;
	const L ln = { (int)threadIdx.x, p.n };
	const size_t off = (size_t)s * p.n;
	float x[L::E];
	ln.load(x, (const T*)p.a + off, 0.f);
	float t[1] = { 0.f };
#pragma unroll
	for (int k = 0; k < L::E; k++) t[0] += x[k];
	row_reduce<true, false, 1>(t, red);
	const float mean = t[0] * p.inv_n;
	float v[1] = { 0.f };
#pragma unroll
	for (int k = 0; k < L::E; k++) {
		x[k] = ln.has(k) ? x[k] - mean : 0.f;
		v[0] = __builtin_fmaf(x[k], x[k], v[0]);
	}
	row_reduce<true, false, 1>(v, red + 8);
	const float inv_std = 1.f / sqrtf(__builtin_fmaf(v[0], p.inv_n, p.epsilon));
	if (threadIdx.x == 0) {
		((P*)p.mean)[s] = (P)f32_rounded(mean);
		((P*)p.inv_std)[s] = (P)f32_rounded(inv_std);
	}
	const P* const scale = (const P*)p.scale;
	const P* const bias = (const P*)p.bias;
	const bool whole = VEC && p.inner8;
#pragma unroll
	for (int k = 0; k < L::E; k++) {
		const unsigned ch = (scale || bias) && ln.has(k) ? channel_of(off, ln.col(k), whole, (unsigned)p.inner, (unsigned)p.C) : 0;
		float y = x[k] * inv_std;
		if (scale) y = y * (float)scale[ch];
		if (bias) y = y + (float)bias[ch];
		x[k] = y;
	}
	ln.store((T*)p.out + off, x);
}
// h alone: s1 = sum gss and s2 = sum ah gss over the run, as the row kernels have them
template <class T, class P, int NV, bool VEC>
__global__ void __launch_bounds__(GN_THREADS) planar_reg_bwd_kernel(const args_t p)
{
#pragma clang fp contract(off)
	typedef lane_t<NV, true, VEC> L;
	__shared__ float red[rows::RED_FLOATS];
	const int s = blockIdx.x;
	const L ln = { (int)threadIdx.x, p.n };
	const size_t off = (size_t)s * p.n;
	const float mean = (float)((const P*)p.mean_in)[s], inv_std = (float)((const P*)p.inv_std_in)[s];
	float a[L::E], g[L::E];
	ln.load(a, (const T*)p.a + off, 0.f);
	ln.load(g, (const T*)p.g + off, 0.f);
	const P* const scale = (const P*)p.scale;
	const bool whole = VEC && p.inner8;
	float t[2] = { 0.f, 0.f };
#pragma unroll
	for (int k = 0; k < L::E; k++) {
		a[k] = ln.has(k) ? (a[k] - mean) * inv_std : 0.f; // ah
		if (scale) g[k] = g[k] * (ln.has(k) ? (float)scale[channel_of(off, ln.col(k), whole, (unsigned)p.inner, (unsigned)p.C)] : 0.f);
		g[k] = g[k] * inv_std; // gss
		t[0] += g[k];
		t[1] = __builtin_fmaf(a[k], g[k], t[1]);
	}
	row_reduce<true, false, 2>(t, red);
#pragma unroll
	for (int k = 0; k < L::E; k++) g[k] = __builtin_fmaf(-p.inv_n, __builtin_fmaf(a[k], t[1], t[0]), g[k]);
	ln.store((T*)p.out + off, g);
}
static inline bool is_reg(const shape_t& s) { return !s.inter && s.n <= GN_REG_MAX; }
// CALL(NV) for the vectors a lane holds: 1, 2, 4 or 8
#define GN_REG_DISPATCH(n, CALL) do { \
		const int nv_ = ((n) + GN_THREADS * GN_LANE - 1) / (GN_THREADS * GN_LANE); \
		if (nv_ <= 1) CALL(1); else if (nv_ == 2) CALL(2); else if (nv_ <= 4) CALL(4); else CALL(8); \
	} while (0)

// ---- inter -------------------------------------------------------------------------------------------------------------------------------------------------------
// A workgroup is cvt = 1 << cvt_log2 channel-vector columns x 256 / cvt pixel-row phases (one phase when C has more than 256 vectors: a lane then walks
// several columns, one after the other).  W = 8: 16-byte vectors; W = 1: the scalar instance.  rows of phase ph in a slice of `nrows`:
__device__ __forceinline__ int phase_rows(const int nrows, const int ph, const int phases) { return nrows > ph ? (nrows - ph + phases - 1) / phases : 0; }
template <class T, int W> struct vec_t {
	float x[W];
	__device__ __forceinline__ void load(const T* const q)
	{
		if constexpr (W == GN_LANE) {
			raw8<T> r;
			r.load(q);
#pragma unroll
			for (int e = 0; e < W; e++) x[e] = r.get(e);
		} else x[0] = (float)q[0];
	}
	// (x holds arithmetic results: rounded once)
	__device__ __forceinline__ void store(T* const q) const
	{
		if constexpr (W == GN_LANE) {
			raw8<T> r;
#pragma unroll
			for (int e = 0; e < W; e++) r.set(e, f32_rounded(x[e]));
			r.store(q);
		} else q[0] = (T)f32_rounded(x[0]);
	}
};
// grid outer x slices.  Forward: Welford per lane and channel, (count, mean, M2) per (statistic, slice).  BWD: A, B per (image, slice, channel).
template <class T, class P, int W, bool BWD>
__global__ void __launch_bounds__(GN_THREADS) inter_reduce_kernel(const args_t p)
{
#pragma clang fp contract(off)
	__shared__ float l0[GN_MAX_C], l1[GN_MAX_C]; // [phase][C]
	const int cvt = 1 << p.cvt_log2, phases = GN_THREADS >> p.cvt_log2;
	const int q = threadIdx.x & (cvt - 1), phase = threadIdx.x >> p.cvt_log2;
	const int cv = p.C / W, img = blockIdx.x / p.slices, sl = blockIdx.x % p.slices;
	const int r0 = sl * p.per, r1 = r0 + p.per < p.inner ? r0 + p.per : p.inner;
	for (int cvi = q; cvi < cv; cvi += cvt) {
		const int c0 = cvi * W;
		float u0[W], u1[W], mean[BWD ? W : 1], inv_std[BWD ? W : 1];
#pragma unroll
		for (int e = 0; e < W; e++) u0[e] = u1[e] = 0.f;
		if constexpr (BWD) {
#pragma unroll
			for (int e = 0; e < W; e++) {
				const int s = img * p.G + (c0 + e) / p.cg;
				mean[e] = (float)((const P*)p.mean_in)[s]; inv_std[e] = (float)((const P*)p.inv_std_in)[s];
			}
		}
		float cnt = 0.f;
		for (int r = r0 + phase; r < r1; r += phases) {
			const size_t o = ((size_t)img * p.inner + r) * p.C + c0;
			vec_t<T, W> a;
			a.load((const T*)p.a + o);
			if constexpr (BWD) {
				vec_t<T, W> g;
				g.load((const T*)p.g + o);
#pragma unroll
				for (int e = 0; e < W; e++) {
					u0[e] += g.x[e];
					u1[e] = __builtin_fmaf((a.x[e] - mean[e]) * inv_std[e], g.x[e], u1[e]);
				}
			} else {
				cnt += 1.f;
				const float rc = 1.f / cnt;
#pragma unroll
				for (int e = 0; e < W; e++) { // u0: mean, u1: M2
					const float d = a.x[e] - u0[e];
					u0[e] = __builtin_fmaf(d, rc, u0[e]);
					u1[e] = __builtin_fmaf(d, a.x[e] - u0[e], u1[e]);
				}
			}
		}
#pragma unroll
		for (int e = 0; e < W; e++) { l0[phase * p.C + c0 + e] = u0[e]; l1[phase * p.C + c0 + e] = u1[e]; }
	}
	__syncthreads();
	if constexpr (BWD) {
		for (int c = threadIdx.x; c < p.C; c += GN_THREADS) {
			float A = l0[c], B = l1[c];
			for (int ph = 1; ph < phases; ph++) { A += l0[ph * p.C + c]; B += l1[ph * p.C + c]; }
			const size_t o = ((size_t)img * p.sum_slices + sl) * p.C + c;
			p.part[o] = A;
			p.part[p.sums_floats + o] = B;
		}
	} else {
		for (int grp = threadIdx.x; grp < p.G; grp += GN_THREADS) { // channel by channel, phase by phase; the two passes of fold_stats
			float cn = 0.f, sm = 0.f, m2 = 0.f;
			for (int c = grp * p.cg; c < (grp + 1) * p.cg; c++)
				for (int ph = 0; ph < phases; ph++) { const float k = (float)phase_rows(r1 - r0, ph, phases); cn += k; sm = __builtin_fmaf(k, l0[ph * p.C + c], sm); }
			const float m = sm / cn;
			for (int c = grp * p.cg; c < (grp + 1) * p.cg; c++)
				for (int ph = 0; ph < phases; ph++) { const float d = l0[ph * p.C + c] - m; m2 += __builtin_fmaf((float)phase_rows(r1 - r0, ph, phases) * d, d, l1[ph * p.C + c]); }
			float* const o = p.part + ((size_t)(img * p.G + grp) * p.slices + sl) * 3;
			o[0] = cn; o[1] = m; o[2] = m2;
		}
	}
}
// grid outer x slices: the statistics of the image's groups into LDS, then the slice
template <class T, class P, int W, bool BWD>
__global__ void __launch_bounds__(GN_THREADS) inter_apply_kernel(const args_t p)
{
#pragma clang fp contract(off)
	__shared__ float sm[BWD ? 4 : 2][GN_MAX_G];
	const int cvt = 1 << p.cvt_log2, phases = GN_THREADS >> p.cvt_log2;
	const int q = threadIdx.x & (cvt - 1), phase = threadIdx.x >> p.cvt_log2;
	const int cv = p.C / W, img = blockIdx.x / p.slices, sl = blockIdx.x % p.slices;
	const int r0 = sl * p.per, r1 = r0 + p.per < p.inner ? r0 + p.per : p.inner;
	if constexpr (BWD) {
		for (int grp = threadIdx.x; grp < p.G; grp += GN_THREADS) {
			const int s = img * p.G + grp;
			sm[0][grp] = (float)((const P*)p.mean_in)[s]; sm[1][grp] = (float)((const P*)p.inv_std_in)[s];
			sm[2][grp] = p.s12[2 * (size_t)s]; sm[3][grp] = p.s12[2 * (size_t)s + 1];
		}
	} else { // lpg lanes per group (a power of two, one wave's at most), 256 / lpg groups at a time: the two passes of fold_stats, each lane's share of the
		// slices first, then across the group's lanes in a fixed order.  Every lane takes part in the exchanges, also one whose group does not exist.
		int lpg = 64;
		while (lpg > 1 && lpg * p.G > GN_THREADS) lpg >>= 1;
		const int sub = threadIdx.x & (lpg - 1);
		for (int g0 = 0; g0 < p.G; g0 += GN_THREADS / lpg) {
			const int grp = g0 + (int)threadIdx.x / lpg;
			const bool live = grp < p.G;
			const int s = img * p.G + (live ? grp : 0);
			const float* const f = p.part + (size_t)s * p.slices * 3;
			float cn = 0.f, sum = 0.f, m2 = 0.f;
			if (live) for (int i = sub; i < p.slices; i += lpg) { cn += f[3 * i]; sum = __builtin_fmaf(f[3 * i], f[3 * i + 1], sum); }
			for (int o = lpg >> 1; o > 0; o >>= 1) { cn += __shfl_xor(cn, o); sum += __shfl_xor(sum, o); }
			const float mean = live ? sum / cn : 0.f;
			if (live) for (int i = sub; i < p.slices; i += lpg) { const float d = f[3 * i + 1] - mean; m2 += __builtin_fmaf(f[3 * i] * d, d, f[3 * i + 2]); }
			for (int o = lpg >> 1; o > 0; o >>= 1) m2 += __shfl_xor(m2, o);
			const float inv_std = 1.f / sqrtf(__builtin_fmaf(m2, p.inv_n, p.epsilon));
			if (live && sub == 0) {
				sm[0][grp] = mean; sm[1][grp] = inv_std;
				if (sl == 0) {
					((P*)p.mean)[s] = (P)f32_rounded(mean);
					((P*)p.inv_std)[s] = (P)f32_rounded(inv_std);
				}
			}
		}
	}
	__syncthreads();
	const P* const scale = (const P*)p.scale;
	const P* const bias = (const P*)p.bias;
	for (int cvi = q; cvi < cv; cvi += cvt) {
		const int c0 = cvi * W;
		float mean[W], inv_std[W], sc[W], t0[W], t1[W]; // forward: t0 = bias; BWD: t0 = s1, t1 = s2
#pragma unroll
		for (int e = 0; e < W; e++) {
			const int grp = (c0 + e) / p.cg;
			mean[e] = sm[0][grp]; inv_std[e] = sm[1][grp];
			sc[e] = scale ? (float)scale[c0 + e] : 1.f;
			if constexpr (BWD) { t0[e] = sm[2][grp]; t1[e] = sm[3][grp]; }
			else { t0[e] = bias ? (float)bias[c0 + e] : 0.f; t1[e] = 0.f; }
		}
		for (int r = r0 + phase; r < r1; r += phases) {
			const size_t o = ((size_t)img * p.inner + r) * p.C + c0;
			vec_t<T, W> a;
			a.load((const T*)p.a + o);
			if constexpr (BWD) {
				vec_t<T, W> g;
				g.load((const T*)p.g + o);
#pragma unroll
				for (int e = 0; e < W; e++) {
					const float ah = (a.x[e] - mean[e]) * inv_std[e];
					float gs = g.x[e];
					if (scale) gs = gs * sc[e];
					gs = gs * inv_std[e];
					a.x[e] = __builtin_fmaf(-p.inv_n, __builtin_fmaf(ah, t1[e], t0[e]), gs);
				}
			} else {
#pragma unroll
				for (int e = 0; e < W; e++) {
					float y = (a.x[e] - mean[e]) * inv_std[e];
					if (scale) y = y * sc[e];
					if (bias) y = y + t0[e];
					a.x[e] = y;
				}
			}
			a.store((T*)p.out + o);
		}
	}
}

// ---- the backward fold, both layouts, over the sums [outer][sum_slices][C].  Workgroups [0, stat_wgs): one statistic each, its 256 threads over the flat
// (slice, channel of the group) items -- s1 = inv_std sum scale A, s2 = inv_std sum scale B.  The others: 16 channels x 16 phases each over all outer x sum_slices
// rows (fold_slices / fold_phases of common.h) -- dbias = sum A, dscale = sum B.  Every order is fixed.
template <class P>
__global__ void __launch_bounds__(GN_THREADS) fold_kernel(const args_t p)
{
#pragma clang fp contract(off)
	__shared__ float red[2][FOLD_PH][FOLD_CH];
	if ((int)blockIdx.x < p.stat_wgs) {
		const int s = blockIdx.x, o = s / p.G, c0 = (s % p.G) * p.cg;
		const float* const A = p.part + (size_t)o * p.sum_slices * p.C + c0;
		const int items = p.cg * p.sum_slices;
		float v[2] = { 0.f, 0.f };
		for (int f = threadIdx.x; f < items; f += GN_THREADS) {
			const int sl = f / p.cg, c = f - sl * p.cg;
			const size_t q = (size_t)sl * p.C + c;
			const float sc = p.scale ? (float)((const P*)p.scale)[c0 + c] : 1.f;
			v[0] = __builtin_fmaf(sc, A[q], v[0]);
			v[1] = __builtin_fmaf(sc, A[p.sums_floats + q], v[1]);
		}
		row_reduce<true, false, 2>(v, &red[0][0][0]);
		if (threadIdx.x == 0) {
			const float inv_std = (float)((const P*)p.inv_std_in)[s];
			p.s12[2 * (size_t)s] = inv_std * v[0];
			p.s12[2 * (size_t)s + 1] = inv_std * v[1];
		}
		return;
	}
	const int ch = threadIdx.x & (FOLD_CH - 1), phase = threadIdx.x / FOLD_CH;
	const int c = ((int)blockIdx.x - p.stat_wgs) * FOLD_CH + ch;
	const long rows = (long)p.outer * p.sum_slices;
	red[0][phase][ch] = c < p.C && p.dbias ? fold_slices(p.part, rows, p.C, c, phase) : 0.f;
	red[1][phase][ch] = c < p.C && p.dscale ? fold_slices(p.part + p.sums_floats, rows, p.C, c, phase) : 0.f;
	__syncthreads();
	if (phase == 0 && c < p.C) {
		if (p.dbias) ((P*)p.dbias)[c] = (P)f32_rounded(fold_phases(red[0], ch));
		if (p.dscale) ((P*)p.dscale)[c] = (P)f32_rounded(fold_phases(red[1], ch));
	}
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------------------------------------
template <class P> static inline const char* type_tag(void) { return sizeof(P) == 2 ? "hh" : "hf"; }
static inline bool all_aligned(const void* const* const bases, const int count)
{
	for (int i = 0; i < count; i++) if (bases[i] && !aligned16(bases[i])) return false;
	return true;
}
static inline void fill_shape(args_t& p, const shape_t& s)
{
	p.outer = s.outer; p.C = s.C; p.G = s.G; p.cg = s.cg; p.inner = s.inner; p.n = s.n; p.R = s.R;
	p.inner8 = s.inner % GN_LANE == 0;
	p.inv_n = 1.f / (float)s.n;
	const slice_plan_t mp = map_plan(s), sp = sums_plan(s);
	p.slices = mp.slices; p.per = mp.per; p.sum_slices = sp.slices; p.sum_per = sp.per;
	p.sums_floats = bwd_sums_floats(s);
}
// inter: the channel-vector columns of a workgroup, a power of two
static inline int cvt_log2_of(const int cv) { int l = 0; while ((1 << l) < cv && l < 8) l++; return l; }
static inline bool shape_served(const shape_t& s) { return s.R > 0 && s.n > 0 && (!s.inter || (s.C <= GN_MAX_C && s.G <= GN_MAX_G)); }

// `p`: pointers and epsilon filled in by the caller
template <class P>
static int forward(args_t p, const shape_t& s, ccv_nnc_stream_context_t* const ctx)
{
	typedef half_t T;
	if (!shape_served(s)) return CCV_NNC_EXEC_INVALID;
	fill_shape(p, s);
	if (!is_reg(s)) {
		p.part = (float*)workspace_of(ctx, fwd_workspace_bytes(s));
		if (!p.part) return CCV_NNC_EXEC_OOM;
	}
	const void* const bases[2] = { p.a, p.out };
	const bool vec = all_aligned(bases, 2) && (s.inter ? s.C : s.n) % GN_LANE == 0;
	p.cvt_log2 = cvt_log2_of(vec ? s.C / GN_LANE : s.C);
	hipStream_t stream = stream_of(ctx);
	const dim3 grid((unsigned)((long)p.slices * (s.inter ? s.outer : s.R)));
	const double count = (double)s.R * s.n, params = sizeof(P) * (2.0 * s.R + (p.scale ? s.C : 0) + (p.bias ? s.C : 0));
	char name[96];
	note_kernel("gnorm_fwd");
	if (is_reg(s)) {
		snprintf(name, sizeof(name), "gnorm_fwd_%s|nnc::gnorm::planar_reg_fwd_kernel", type_tag<P>());
		ProfScope prof(name, 8.0 * count, count * 2 * sizeof(T) + params, s.R, s.n, 1, 1, 1, stream);
#define GN_CALL(NV) do { \
			if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_reg_fwd_kernel<T, P, NV, true>), dim3(s.R), dim3(GN_THREADS), 0, stream, p); \
			else hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_reg_fwd_kernel<T, P, NV, false>), dim3(s.R), dim3(GN_THREADS), 0, stream, p); \
		} while (0)
		GN_REG_DISPATCH(s.n, GN_CALL);
#undef GN_CALL
		HIP_ENFORCE(hipGetLastError());
		return CCV_NNC_EXEC_SUCCESS;
	}
	{
		snprintf(name, sizeof(name), "gnorm_fwd_%s|nnc::gnorm::%s_split_stats_kernel", type_tag<P>(), s.inter ? "inter" : "planar");
		ProfScope prof(name, 4.0 * count, count * sizeof(T) + 12.0 * s.R * p.slices, s.R, s.n, 1, 1, p.slices, stream);
		if (s.inter) {
			if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_reduce_kernel<T, P, GN_LANE, false>), grid, dim3(GN_THREADS), 0, stream, p);
			else hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_reduce_kernel<T, P, 1, false>), grid, dim3(GN_THREADS), 0, stream, p);
		} else if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_stats_kernel<T, true>), grid, dim3(GN_THREADS), 0, stream, p);
		else hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_stats_kernel<T, false>), grid, dim3(GN_THREADS), 0, stream, p);
		HIP_ENFORCE(hipGetLastError());
	}
	{
		snprintf(name, sizeof(name), "gnorm_fwd_%s|nnc::gnorm::%s_split_apply_kernel", type_tag<P>(), s.inter ? "inter" : "planar");
		ProfScope prof(name, 4.0 * count, count * 2 * sizeof(T) + params, s.R, s.n, 1, 1, p.slices, stream);
		if (s.inter) {
			if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_apply_kernel<T, P, GN_LANE, false>), grid, dim3(GN_THREADS), 0, stream, p);
			else hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_apply_kernel<T, P, 1, false>), grid, dim3(GN_THREADS), 0, stream, p);
		} else if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_apply_kernel<T, P, true, false>), grid, dim3(GN_THREADS), 0, stream, p);
		else hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_apply_kernel<T, P, false, false>), grid, dim3(GN_THREADS), 0, stream, p);
		HIP_ENFORCE(hipGetLastError());
	}
	return CCV_NNC_EXEC_SUCCESS;
}

// p.out (h), p.dscale, p.dbias: each may be null
template <class P>
static int backward(args_t p, const shape_t& s, ccv_nnc_stream_context_t* const ctx)
{
	typedef half_t T;
	if (!p.out && !p.dscale && !p.dbias) return CCV_NNC_EXEC_SUCCESS;
	if (!shape_served(s)) return CCV_NNC_EXEC_INVALID;
	fill_shape(p, s);
	const bool params = p.dscale || p.dbias;
	if (!is_reg(s) || params) {
		p.part = (float*)workspace_of(ctx, bwd_workspace_bytes(s));
		if (!p.part) return CCV_NNC_EXEC_OOM;
		p.s12 = p.part + 2 * p.sums_floats;
	}
	const void* const bases[3] = { p.a, p.g, p.out };
	const bool aligned = all_aligned(bases, 3);
	const bool vec = aligned && (s.inter ? s.C : s.n) % GN_LANE == 0, vec_sums = aligned && (s.inter ? s.C : s.inner) % GN_LANE == 0;
	p.cvt_log2 = cvt_log2_of(vec ? s.C / GN_LANE : s.C);
	p.stat_wgs = p.out ? s.R : 0;
	hipStream_t stream = stream_of(ctx);
	const double count = (double)s.R * s.n, sums_bytes = sizeof(float) * 2.0 * (double)p.sums_floats;
	const char* const lay = s.inter ? "inter" : "planar";
	char name[96];
	note_kernel("gnorm_bwd");
	if (is_reg(s) && !params) { // h alone
		snprintf(name, sizeof(name), "gnorm_bwd_%s|nnc::gnorm::planar_reg_bwd_kernel", type_tag<P>());
		ProfScope prof(name, 12.0 * count, count * 3 * sizeof(T) + sizeof(P) * (2.0 * s.R + (p.scale ? s.C : 0)), s.R, s.n, 1, 1, 1, stream);
#define GN_CALL(NV) do { \
			if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_reg_bwd_kernel<T, P, NV, true>), dim3(s.R), dim3(GN_THREADS), 0, stream, p); \
			else hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_reg_bwd_kernel<T, P, NV, false>), dim3(s.R), dim3(GN_THREADS), 0, stream, p); \
		} while (0)
		GN_REG_DISPATCH(s.n, GN_CALL);
#undef GN_CALL
		HIP_ENFORCE(hipGetLastError());
		return CCV_NNC_EXEC_SUCCESS;
	}
	{
		snprintf(name, sizeof(name), "gnorm_bwd_%s|nnc::gnorm::%s_split_sums_kernel", type_tag<P>(), lay);
		ProfScope prof(name, 4.0 * count, count * 2 * sizeof(T) + sums_bytes + sizeof(P) * 2.0 * s.R, s.R, s.n, 1, 1, p.sum_slices, stream);
		if (s.inter) {
			const dim3 grid((unsigned)((long)p.sum_slices * s.outer));
			if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_reduce_kernel<T, P, GN_LANE, true>), grid, dim3(GN_THREADS), 0, stream, p);
			else hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_reduce_kernel<T, P, 1, true>), grid, dim3(GN_THREADS), 0, stream, p);
		} else {
			const dim3 grid((unsigned)(((long)s.outer * s.C * p.sum_slices + 3) / 4));
			if (vec_sums) hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_sums_kernel<T, P, true>), grid, dim3(GN_THREADS), 0, stream, p);
			else hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_sums_kernel<T, P, false>), grid, dim3(GN_THREADS), 0, stream, p);
		}
		HIP_ENFORCE(hipGetLastError());
	}
	{
		snprintf(name, sizeof(name), "gnorm_bwd_%s|nnc::gnorm::%s_split_fold_kernel", type_tag<P>(), lay);
		ProfScope prof(name, 2.0 * (double)p.sums_floats, sums_bytes * (p.out && params ? 2 : 1) + sizeof(P) * (params ? 2.0 * s.C : 0.0) + 8.0 * p.stat_wgs, s.R, s.C, 1, 1, p.sum_slices, stream);
		hipLaunchKernelGGL(HIP_KERNEL_NAME(fold_kernel<P>), dim3(p.stat_wgs + (params ? (s.C + FOLD_CH - 1) / FOLD_CH : 0)), dim3(GN_THREADS), 0, stream, p);
		HIP_ENFORCE(hipGetLastError());
	}
	if (p.out) {
		snprintf(name, sizeof(name), "gnorm_bwd_%s|nnc::gnorm::%s_split_apply_kernel", type_tag<P>(), lay);
		ProfScope prof(name, 8.0 * count, count * 3 * sizeof(T) + sizeof(P) * (2.0 * s.R + (p.scale ? s.C : 0)), s.R, s.n, 1, 1, p.slices, stream);
		const dim3 grid((unsigned)((long)p.slices * (s.inter ? s.outer : s.R)));
		if (s.inter) {
			if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_apply_kernel<T, P, GN_LANE, true>), grid, dim3(GN_THREADS), 0, stream, p);
			else hipLaunchKernelGGL(HIP_KERNEL_NAME(inter_apply_kernel<T, P, 1, true>), grid, dim3(GN_THREADS), 0, stream, p);
		} else if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_apply_kernel<T, P, true, true>), grid, dim3(GN_THREADS), 0, stream, p);
		else hipLaunchKernelGGL(HIP_KERNEL_NAME(planar_apply_kernel<T, P, false, true>), grid, dim3(GN_THREADS), 0, stream, p);
		HIP_ENFORCE(hipGetLastError());
	}
	return CCV_NNC_EXEC_SUCCESS;
}

} // namespace gnorm
} // namespace nnc
