// Row kernels: LAYER_NORM, RMSNORM and plain SOFTMAX, forward and backward, over dense [rows][n] maps of element type T (a, b, g, h) with per-column parameters
// and per-row statistics of type P (scale, bias, saved_mean, saved_inv_std, dscale, dbias).  Each type is _Float16 or float; only T = _Float16 is registered
// (half_stage.cpp g_native_half, tunable ROW_HALF_NATIVE) -- the fp32 commands keep the kernels of cmd_rownorm.cpp / cmd_act_opt.cpp and their bits.
// Semantics: cmd_rownorm.cpp:1-12 and cmd_act_opt.cpp:10.
//
// Arithmetic: fp32 throughout, operands widened on load (exact), a value rounded to half exactly once, where it is stored (f32_rounded keeps the compiler from
// merging the last multiply into the conversion).  Contraction is written out as in optim.h: the pragma turns it off and every fma below is spelled as one, so
// the vector lanes, the scalar route and the emulator build carry the same bits.
// Memory: a row is read from HBM ONCE and lives in registers for every pass; every output is written once.  Two forms, chosen by n alone:
//   wave form  n <= ROW_WAVE_MAX          one wave per row, four rows per 256-thread workgroup; reductions by cross-lane shuffles only (no LDS, no barrier)
//   wg form    ROW_WAVE_MAX < n <= ROW_REG_MAX   256 threads per row; per reduction one LDS exchange (one barrier), the four waves combined in a fixed order
// n > ROW_REG_MAX is not served (the predicates in cmd_rownorm.cpp / cmd_act_opt.cpp refuse it: fp32 images as before).
// Columns of a lane: with n a multiple of 8 and every base 16-byte aligned, lane l holds the 16-byte vectors l, l + LANES, ... of the row (ROW_LANE = 8 elements
// each, whatever the type: raw8 of optim.h); otherwise row starts are not aligned and the scalar instance of the same kernel (VEC = false) takes one element per load, lane l holding the columns
// l, l + LANES, ...  Either way a lane owns the SAME columns in every row, and reads all of its elements of a row before it writes any: b = a and h = g are fine.
// Parameter gradients (two launches, no atomics, the same bits every run): a wave (wave form) or a workgroup (wg form) walks one contiguous chunk of rows
// (row_chunk_plan), each lane keeping sum ah g and sum g of its columns in fp32 registers, and writes partial[2][chunk][n] at the end; chan_fold_kernel
// (chan_sums.h) folds both arrays in one launch, in a fixed order, into half or fp32 outputs.  The next row of a chunk is fetched while the current one is reduced.
// No kernel takes a per-launch host counter: they replay unchanged inside a captured graph.
#pragma once
#include "chan_sums.h"
#include "optim.h"

namespace nnc {
namespace rows {

using optim::raw8;
typedef _Float16 half_t;

constexpr int ROW_THREADS = 256;
constexpr int ROW_LANE = 8; // elements of one vector access
constexpr int ROW_WAVE_MAX = 1024; // longest row of the wave form (tests/test_rows_half.py reads this line)
constexpr int ROW_REG_MAX = 8192; // longest row served at all (tests/test_rows_half.py reads this line)
constexpr int ROW_CHUNK_ROWS = 16; // rows of one chunk of the backward pass with parameter gradients (tests/test_rows_half.py reads this line)
constexpr int ROW_MAX_CHUNKS = 2048; // ... until there would be more chunks than this: then the chunks grow
static_assert(ROW_WAVE_MAX == 64 * 2 * ROW_LANE && ROW_REG_MAX == ROW_THREADS * 4 * ROW_LANE, "a lane holds at most two (wave form) / four (wg form) vectors");

// ---- the chunk plan of the backward pass with parameter gradients, and what it asks of the workspace ---------------------------------------------------
struct row_chunk_plan_t { int chunks, rows_per_chunk; };
static inline row_chunk_plan_t row_chunk_plan(const int rows)
{
	row_chunk_plan_t p;
	p.rows_per_chunk = (rows + ROW_MAX_CHUNKS - 1) / ROW_MAX_CHUNKS;
	if (p.rows_per_chunk < ROW_CHUNK_ROWS) p.rows_per_chunk = ROW_CHUNK_ROWS;
	p.chunks = (rows + p.rows_per_chunk - 1) / p.rows_per_chunk;
	return p;
}
static inline size_t row_partials_bytes(const int rows, const int n) { return sizeof(float) * 2 * (size_t)row_chunk_plan(rows).chunks * (size_t)n; } // [2][chunks][n]
// vectors a lane holds: wave form 1 (n <= 512) or 2, wg form 1 (n <= 2048), 2 (n <= 4096) or 4
static inline bool row_is_wg(const int n) { return n > ROW_WAVE_MAX; }
static inline int row_vectors(const int n)
{
	const int per = (row_is_wg(n) ? ROW_THREADS : 64) * ROW_LANE;
	const int nv = (n + per - 1) / per;
	return nv == 3 ? 4 : nv;
}

// ---- a lane's share of one row ---------------------------------------------------------------------------------------------------------------------------
// E = NV * ROW_LANE values; element k is column col(k).  VEC: the vector route.  (An instance of its own, not a flag: with both routes in one body the
// compiler kept the scalar route's per-element addresses live across the row loop -- 180 to 250 registers in the backward kernels.)
template <int NV, bool WG, bool VEC>
struct lane_t {
	static constexpr int LANES = WG ? ROW_THREADS : 64;
	static constexpr int E = NV * ROW_LANE;
	int lane, n;
	static constexpr bool vec = VEC;
	__device__ __forceinline__ int col(const int k) const { return vec ? (((k / ROW_LANE) * LANES + lane) * ROW_LANE + (k % ROW_LANE)) : (k * LANES + lane); }
	__device__ __forceinline__ bool has(const int k) const { return col(k) < n; }
	// x[k] = p[col(k)], `fill` beyond the row
	template <class TT>
	__device__ __forceinline__ void load(float (&x)[E], const TT* const p, const float fill) const
	{
		if constexpr (VEC) {
#pragma unroll
			for (int v = 0; v < NV; v++) {
				const int c = (v * LANES + lane) * ROW_LANE;
				if (c < n) {
					raw8<TT> r;
					r.load(p + c);
#pragma unroll
					for (int e = 0; e < ROW_LANE; e++) x[v * ROW_LANE + e] = r.get(e);
				} else {
#pragma unroll
					for (int e = 0; e < ROW_LANE; e++) x[v * ROW_LANE + e] = fill;
				}
			}
		} else {
#pragma unroll
			for (int k = 0; k < E; k++) { const int c = k * LANES + lane; x[k] = c < n ? (float)p[c] : fill; }
		}
	}
	// The same in two steps, for a row that is fetched one iteration ahead: the loads are issued into `raw` as they lie in memory and widened when the row's
	// turn comes (a widened value would have to wait for its load on the spot).
	template <class TT> struct raw_t { raw8<TT> v[VEC ? NV : 1]; TT s[VEC ? 1 : E]; };
	template <class TT>
	__device__ __forceinline__ void fetch(raw_t<TT>& raw, const TT* const p) const
	{
		if constexpr (VEC) {
#pragma unroll
			for (int v = 0; v < NV; v++) {
				const int c = (v * LANES + lane) * ROW_LANE;
				if (c < n) raw.v[v].load(p + c);
			}
		} else {
#pragma unroll
			for (int k = 0; k < E; k++) { const int c = k * LANES + lane; if (c < n) raw.s[k] = p[c]; }
		}
	}
	template <class TT>
	__device__ __forceinline__ void widen(float (&x)[E], const raw_t<TT>& raw, const float fill) const
	{
#pragma unroll
		for (int k = 0; k < E; k++) {
			float v;
			if constexpr (VEC) v = raw.v[k / ROW_LANE].get(k % ROW_LANE); else v = (float)raw.s[k];
			x[k] = has(k) ? v : fill;
		}
	}
	// a per-column parameter: n elements (inc 1; `pvec`: 16-byte aligned, so the vector route may take it whole) or one for all (inc 0)
	template <class TT>
	__device__ __forceinline__ void load_param(float (&x)[E], const TT* const p, const int inc, const bool pvec, const float fill) const
	{
		if (!inc) {
			const float v = (float)p[0];
#pragma unroll
			for (int k = 0; k < E; k++) x[k] = v;
		} else if (VEC && pvec) load(x, p, fill);
		else {
#pragma unroll
			for (int k = 0; k < E; k++) { const int c = col(k); x[k] = c < n ? (float)p[c] : fill; }
		}
	}
	// p[col(k)] = x[k], rounded once (x[k] is an arithmetic result: f32_rounded keeps the conversion apart from it)
	template <class TT>
	__device__ __forceinline__ void store(TT* const p, const float (&x)[E]) const
	{
		if constexpr (VEC) {
#pragma unroll
			for (int v = 0; v < NV; v++) {
				const int c = (v * LANES + lane) * ROW_LANE;
				if (c < n) {
					raw8<TT> r;
#pragma unroll
					for (int e = 0; e < ROW_LANE; e++) r.set(e, f32_rounded(x[v * ROW_LANE + e]));
					r.store(p + c);
				}
			}
		} else {
#pragma unroll
			for (int k = 0; k < E; k++) { const int c = k * LANES + lane; if (c < n) p[c] = (TT)f32_rounded(x[k]); }
		}
	}
};

// ---- reductions over a row: NR values at once.  Wave form: shuffles.  Wg form: shuffles, then ONE exchange through `red` (NR x 4 floats nobody else is
// reading: the callers alternate between two areas from row to row, so the barrier of the next reduction separates a slot's readers from its next writer)
template <bool WG, bool IS_MAX, int NR>
__device__ __forceinline__ void row_reduce(float (&v)[NR], float* const red)
{
#pragma clang fp contract(off)
	for (int o = 32; o > 0; o >>= 1)
#pragma unroll
		for (int r = 0; r < NR; r++) { const float w = __shfl_xor(v[r], o); v[r] = IS_MAX ? fmaxf(v[r], w) : v[r] + w; }
	if (WG) {
		if ((threadIdx.x & 63) == 0)
#pragma unroll
			for (int r = 0; r < NR; r++) red[r * 4 + (threadIdx.x >> 6)] = v[r];
		__syncthreads();
#pragma unroll
		for (int r = 0; r < NR; r++) {
			const float a = red[r * 4], b = red[r * 4 + 1], c = red[r * 4 + 2], d = red[r * 4 + 3];
			v[r] = IS_MAX ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : (a + b) + (c + d);
		}
	}
}
constexpr int RED_FLOATS = 2 * 2 * 4; // two areas x at most two values x four waves

// which rows this wave (wave form) / workgroup (wg form) walks: chunk c = rows [c * rows_per_chunk, ...)
template <bool WG>
__device__ __forceinline__ void row_span(const int rows, const int rows_per_chunk, long* const r0, long* const r1)
{
	const long c = WG ? (long)blockIdx.x : (long)blockIdx.x * 4 + (threadIdx.x >> 6);
	*r0 = c * rows_per_chunk;
	*r1 = *r0 + rows_per_chunk < rows ? *r0 + rows_per_chunk : rows;
}
template <bool WG> __device__ __forceinline__ int row_lane(void) { return WG ? (int)threadIdx.x : (int)(threadIdx.x & 63); }

struct norm_args_t {
	const void *a, *g, *scale, *bias, *mean_in, *inv_std_in; // backward reads the statistics, forward writes them
	void *b, *h, *mean, *inv_std;
	float* partial; // [2][chunks][n]: sum ah g, sum g
	int scale_inc, bias_inc, scale_vec, bias_vec;
	int rows, n, rows_per_chunk, chunks, vec;
	float inv_n, epsilon;
};

// ---- LAYER_NORM (CENTER) / RMSNORM forward: b = (a - mean) inv_std scale + bias, variance two-pass and centred -------------------------------------------
template <class T, class P, bool CENTER, int NV, bool WG, bool VEC>
__global__ void __launch_bounds__(ROW_THREADS) norm_fwd_kernel(const norm_args_t p)
{
#pragma clang fp contract(off)
	typedef lane_t<NV, WG, VEC> L;
	__shared__ float red[WG ? RED_FLOATS : 1];
	long r0, r1;
	row_span<WG>(p.rows, 1, &r0, &r1);
	if (r0 >= r1) return; // (a whole wave of the wave form: no barrier follows)
	const L ln = { row_lane<WG>(), p.n };
	const size_t o = (size_t)r0 * p.n;
	float x[L::E];
	ln.load(x, (const T*)p.a + o, 0.f);
	float mean = 0.f;
	if (CENTER) {
		float s[1] = { 0.f };
#pragma unroll
		for (int k = 0; k < L::E; k++) s[0] += x[k];
		row_reduce<WG, false, 1>(s, red);
		mean = s[0] * p.inv_n;
	}
	float v[1] = { 0.f };
#pragma unroll
	for (int k = 0; k < L::E; k++) {
		x[k] = ln.has(k) ? x[k] - mean : 0.f;
		v[0] = __builtin_fmaf(x[k], x[k], v[0]);
	}
	row_reduce<WG, false, 1>(v, red + 8);
	const float inv_std = 1.f / sqrtf(__builtin_fmaf(v[0], p.inv_n, p.epsilon));
	if (ln.lane == 0) {
		if (CENTER) ((P*)p.mean)[r0] = (P)f32_rounded(mean);
		((P*)p.inv_std)[r0] = (P)f32_rounded(inv_std);
	}
#pragma unroll
	for (int k = 0; k < L::E; k++) x[k] = x[k] * inv_std;
	if (p.scale) {
		float w[L::E];
		ln.load_param(w, (const P*)p.scale, p.scale_inc, p.scale_vec != 0, 1.f);
#pragma unroll
		for (int k = 0; k < L::E; k++) x[k] = x[k] * w[k];
	}
	if (p.bias) {
		float w[L::E];
		ln.load_param(w, (const P*)p.bias, p.bias_inc, p.bias_vec != 0, 0.f);
#pragma unroll
		for (int k = 0; k < L::E; k++) x[k] = x[k] + w[k];
	}
	ln.store((T*)p.b + o, x);
}

// ---- LAYER_NORM / RMSNORM backward over one chunk of rows: ah = (a - mean) inv_std, gss = g scale inv_std, h = gss - (sum gss + ah sum(ah gss)) / n (RMSNORM:
// without sum gss); PARAMS: the chunk's sum ah g and sum g per column.  h may be null (parameter gradients only: no reduction over the row at all) --------------
template <class T, class P, bool CENTER, int NV, bool WG, bool VEC, bool PARAMS>
__global__ void __launch_bounds__(ROW_THREADS) norm_bwd_kernel(const norm_args_t p)
{
#pragma clang fp contract(off)
	typedef lane_t<NV, WG, VEC> L;
	__shared__ float red[WG ? RED_FLOATS : 1];
	long r0, r1;
	row_span<WG>(p.rows, p.rows_per_chunk, &r0, &r1);
	if (r0 >= r1) return;
	const L ln = { row_lane<WG>(), p.n };
	float ds[PARAMS ? L::E : 1], db[PARAMS ? L::E : 1];
	if constexpr (PARAMS) {
#pragma unroll
		for (int k = 0; k < L::E; k++) ds[k] = db[k] = 0.f;
	}
	// The next row's loads are in flight while this row is reduced and stored: a chunk is a chain of dependent rows, and with one row at a time every row paid
	// the whole memory latency (16 384 x 1 024 with parameter gradients: 0.046 ms, against 0.020 ms for h alone at a row per wave).
	typename L::template raw_t<T> ra = {}, rg = {}, na = {}, ng = {};
	ln.fetch(ra, (const T*)p.a + (size_t)r0 * p.n);
	ln.fetch(rg, (const T*)p.g + (size_t)r0 * p.n);
	P mean_r = CENTER ? ((const P*)p.mean_in)[r0] : (P)0, inv_std_r = ((const P*)p.inv_std_in)[r0], mean_n = mean_r, inv_std_n = inv_std_r;
	for (long r = r0; r < r1; r++) {
		const size_t o = (size_t)r * p.n;
		if (r + 1 < r1) {
			ln.fetch(na, (const T*)p.a + o + p.n);
			ln.fetch(ng, (const T*)p.g + o + p.n);
			if (CENTER) mean_n = ((const P*)p.mean_in)[r + 1];
			inv_std_n = ((const P*)p.inv_std_in)[r + 1];
		}
		float a[L::E], g[L::E];
		ln.widen(a, ra, 0.f);
		ln.widen(g, rg, 0.f);
		const float mean = (float)mean_r, inv_std = (float)inv_std_r;
		ra = na; rg = ng; mean_r = mean_n; inv_std_r = inv_std_n;
#pragma unroll
		for (int k = 0; k < L::E; k++) a[k] = ln.has(k) ? (a[k] - mean) * inv_std : 0.f; // ah
		if constexpr (PARAMS) {
#pragma unroll
			for (int k = 0; k < L::E; k++) { ds[k] = __builtin_fmaf(a[k], g[k], ds[k]); db[k] += g[k]; }
		}
		if (!p.h) continue;
		if (p.scale) { // (read again for every row, from L1 / L2: E registers less across the loop)
			float sc[L::E];
			ln.load_param(sc, (const P*)p.scale, p.scale_inc, p.scale_vec != 0, 0.f);
#pragma unroll
			for (int k = 0; k < L::E; k++) g[k] = g[k] * sc[k];
		}
		float s[2] = { 0.f, 0.f };
#pragma unroll
		for (int k = 0; k < L::E; k++) {
			g[k] = g[k] * inv_std; // gss
			if (CENTER) s[0] += g[k];
			s[1] = __builtin_fmaf(a[k], g[k], s[1]);
		}
		row_reduce<WG, false, 2>(s, red + ((r - r0) & 1) * 8);
#pragma unroll
		for (int k = 0; k < L::E; k++) g[k] = __builtin_fmaf(-p.inv_n, __builtin_fmaf(a[k], s[1], s[0]), g[k]);
		ln.store((T*)p.h + o, g);
	}
	if constexpr (PARAMS) {
		const size_t c = (size_t)(r0 / p.rows_per_chunk);
		float* const p0 = p.partial + c * p.n;
		float* const p1 = p.partial + ((size_t)p.chunks + c) * p.n;
		// (sums are stored as they are: f32_rounded on an fp32 store is the value itself)
		ln.store(p0, ds);
		ln.store(p1, db);
	}
}

// ---- SOFTMAX forward: b = expf(a - max) / sum; backward: h = (g - sum g b) b -----------------------------------------------------------------------------
struct softmax_args_t { const void *a, *g, *b_in; void *b, *h; int rows, n, vec; };
template <class T, int NV, bool WG, bool VEC>
__global__ void __launch_bounds__(ROW_THREADS) softmax_fwd_kernel(const softmax_args_t p)
{
#pragma clang fp contract(off)
	typedef lane_t<NV, WG, VEC> L;
	__shared__ float red[WG ? RED_FLOATS : 1];
	long r0, r1;
	row_span<WG>(p.rows, 1, &r0, &r1);
	if (r0 >= r1) return;
	const L ln = { row_lane<WG>(), p.n };
	const size_t o = (size_t)r0 * p.n;
	float x[L::E];
	ln.load(x, (const T*)p.a + o, -INFINITY);
	float m[1] = { x[0] };
#pragma unroll
	for (int k = 1; k < L::E; k++) m[0] = fmaxf(m[0], x[k]);
	row_reduce<WG, true, 1>(m, red);
	float s[1] = { 0.f };
#pragma unroll
	for (int k = 0; k < L::E; k++) {
		x[k] = ln.has(k) ? expf(x[k] - m[0]) : 0.f;
		s[0] += x[k];
	}
	row_reduce<WG, false, 1>(s, red + 8);
	const float inv = 1.f / s[0];
#pragma unroll
	for (int k = 0; k < L::E; k++) x[k] = x[k] * inv;
	ln.store((T*)p.b + o, x);
}
template <class T, int NV, bool WG, bool VEC>
__global__ void __launch_bounds__(ROW_THREADS) softmax_bwd_kernel(const softmax_args_t p)
{
#pragma clang fp contract(off)
	typedef lane_t<NV, WG, VEC> L;
	__shared__ float red[WG ? RED_FLOATS : 1];
	long r0, r1;
	row_span<WG>(p.rows, 1, &r0, &r1);
	if (r0 >= r1) return;
	const L ln = { row_lane<WG>(), p.n };
	const size_t o = (size_t)r0 * p.n;
	float g[L::E], b[L::E];
	ln.load(g, (const T*)p.g + o, 0.f);
	ln.load(b, (const T*)p.b_in + o, 0.f);
	float s[1] = { 0.f };
#pragma unroll
	for (int k = 0; k < L::E; k++) s[0] = __builtin_fmaf(g[k], b[k], s[0]);
	row_reduce<WG, false, 1>(s, red);
#pragma unroll
	for (int k = 0; k < L::E; k++) g[k] = (g[k] - s[0]) * b[k];
	ln.store((T*)p.h + o, g);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------------------
// CALL(NV, WG, VEC) for the form and the vectors per lane that n asks for, and the route
#define ROW_FORM_DISPATCH_(n, CALL, VEC) do { \
		const int nv_ = row_vectors(n); \
		if (row_is_wg(n)) { if (nv_ == 1) CALL(1, true, VEC); else if (nv_ == 2) CALL(2, true, VEC); else CALL(4, true, VEC); } \
		else { if (nv_ == 1) CALL(1, false, VEC); else CALL(2, false, VEC); } \
	} while (0)
#define ROW_FORM_DISPATCH(n, vec, CALL) do { if (vec) ROW_FORM_DISPATCH_(n, CALL, true); else ROW_FORM_DISPATCH_(n, CALL, false); } while (0)
static inline unsigned row_grid(const long spans, const int n) { return (unsigned)(row_is_wg(n) ? spans : (spans + 3) / 4); }
template <class T, class P> static inline const char* row_type_tag(void) { return sizeof(T) == 2 ? (sizeof(P) == 2 ? "hh" : "hf") : (sizeof(P) == 2 ? "fh" : "ff"); }
static inline bool row_vec_ok(const int n, const void* const* const bases, const int count)
{
	if (n % ROW_LANE) return false;
	for (int i = 0; i < count; i++) if (bases[i] && !aligned16(bases[i])) return false;
	return true;
}

// `p`: pointers, increments, rows, n, epsilon filled in by the caller; the plan, the vector flags and the record are made here
template <class T, class P, bool CENTER>
static int norm_fwd(norm_args_t p, ccv_nnc_stream_context_t* const ctx)
{
	if (p.rows == 0) return CCV_NNC_EXEC_SUCCESS;
	if (p.n < 1 || p.n > ROW_REG_MAX) return CCV_NNC_EXEC_INVALID;
	const void* const bases[2] = { p.a, p.b };
	p.vec = row_vec_ok(p.n, bases, 2);
	p.scale_vec = p.scale && aligned16(p.scale);
	p.bias_vec = p.bias && aligned16(p.bias);
	p.inv_n = 1.f / (float)p.n;
	p.rows_per_chunk = 1; p.chunks = p.rows;
	hipStream_t stream = stream_of(ctx);
	char name[96];
	snprintf(name, sizeof(name), "rows_%s_fwd_%s|nnc::rows::%s_norm_fwd_kernel", CENTER ? "layernorm" : "rmsnorm", row_type_tag<T, P>(), row_is_wg(p.n) ? "wg" : "wave");
	note_kernel(CENTER ? "rows_layernorm_fwd" : "rows_rmsnorm_fwd");
	const double count = (double)p.rows * p.n;
	ProfScope prof(name, 8.0 * count, count * 2 * sizeof(T) + sizeof(P) * ((CENTER ? 2.0 : 1.0) * p.rows + (p.scale ? (p.scale_inc ? p.n : 1) : 0) + (p.bias ? (p.bias_inc ? p.n : 1) : 0)), p.rows, p.n, 1, 1, 1, stream);
#define ROW_CALL(NV, WG, VEC) hipLaunchKernelGGL(HIP_KERNEL_NAME(norm_fwd_kernel<T, P, CENTER, NV, WG, VEC>), dim3(row_grid(p.rows, p.n)), dim3(ROW_THREADS), 0, stream, p)
	ROW_FORM_DISPATCH(p.n, p.vec, ROW_CALL);
#undef ROW_CALL
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

// h, dscale, dbias: each may be null; the partials come from the stream's workspace
template <class T, class P, bool CENTER>
static int norm_bwd(norm_args_t p, P* const dscale, P* const dbias, ccv_nnc_stream_context_t* const ctx)
{
	if (p.rows == 0 || (!p.h && !dscale && !dbias)) return CCV_NNC_EXEC_SUCCESS;
	if (p.n < 1 || p.n > ROW_REG_MAX) return CCV_NNC_EXEC_INVALID;
	const bool params = dscale || dbias;
	const void* const bases[3] = { p.a, p.g, p.h };
	p.vec = row_vec_ok(p.n, bases, 3);
	p.scale_vec = p.scale && aligned16(p.scale);
	p.inv_n = 1.f / (float)p.n;
	p.rows_per_chunk = 1; p.chunks = p.rows; p.partial = 0;
	if (params) {
		const row_chunk_plan_t plan = row_chunk_plan(p.rows);
		p.rows_per_chunk = plan.rows_per_chunk; p.chunks = plan.chunks;
		p.partial = (float*)workspace_of(ctx, row_partials_bytes(p.rows, p.n));
		if (!p.partial) return CCV_NNC_EXEC_OOM;
	}
	hipStream_t stream = stream_of(ctx);
	char name[96];
	snprintf(name, sizeof(name), "rows_%s_bwd_%s|nnc::rows::%s_norm_bwd_kernel", CENTER ? "layernorm" : "rmsnorm", row_type_tag<T, P>(), row_is_wg(p.n) ? "wg" : "wave");
	const double count = (double)p.rows * p.n, partial_bytes = params ? (double)row_partials_bytes(p.rows, p.n) : 0.0;
	{
		note_kernel(CENTER ? "rows_layernorm_bwd" : "rows_rmsnorm_bwd");
		ProfScope prof(name, 12.0 * count, count * sizeof(T) * (p.h ? 3 : 2) + partial_bytes + sizeof(P) * ((CENTER ? 2.0 : 1.0) * p.rows + (p.h && p.scale ? (p.scale_inc ? p.n : 1) : 0)), p.rows, p.n, 1, 1, p.chunks, stream);
#define ROW_CALL(NV, WG, VEC) do { \
			if (params) hipLaunchKernelGGL(HIP_KERNEL_NAME(norm_bwd_kernel<T, P, CENTER, NV, WG, VEC, true>), dim3(row_grid(p.chunks, p.n)), dim3(ROW_THREADS), 0, stream, p); \
			else hipLaunchKernelGGL(HIP_KERNEL_NAME(norm_bwd_kernel<T, P, CENTER, NV, WG, VEC, false>), dim3(row_grid(p.chunks, p.n)), dim3(ROW_THREADS), 0, stream, p); \
		} while (0)
		ROW_FORM_DISPATCH(p.n, p.vec, ROW_CALL);
#undef ROW_CALL
		HIP_ENFORCE(hipGetLastError());
	}
	if (params) { // one fold for both arrays; a single wanted gradient takes its array alone
		const float* const p0 = p.partial;
		const float* const p1 = p.partial + (size_t)p.chunks * p.n;
		const bool both = dscale && dbias;
		snprintf(name, sizeof(name), "rows_fold_%s|nnc::chan_fold_kernel", sizeof(P) == 2 ? "h" : "f");
		ProfScope prof(name, (both ? 2.0 : 1.0) * p.chunks * p.n, (both ? 2.0 : 1.0) * (sizeof(float) * (double)p.chunks + sizeof(P)) * p.n, p.chunks, p.n, 1, 1, 1, stream);
		hipLaunchKernelGGL(HIP_KERNEL_NAME(chan_fold_kernel<P>), dim3((p.n + FOLD_CH - 1) / FOLD_CH, both ? 2 : 1), dim3(256), 0, stream, dscale ? p0 : p1, p1, (long)p.chunks, p.n, dscale ? dscale : dbias, dbias, 0);
		HIP_ENFORCE(hipGetLastError());
	}
	return CCV_NNC_EXEC_SUCCESS;
}

template <class T>
static int softmax_fwd(softmax_args_t p, ccv_nnc_stream_context_t* const ctx)
{
	if (p.rows == 0) return CCV_NNC_EXEC_SUCCESS;
	if (p.n < 1 || p.n > ROW_REG_MAX) return CCV_NNC_EXEC_INVALID;
	const void* const bases[2] = { p.a, p.b };
	p.vec = row_vec_ok(p.n, bases, 2);
	hipStream_t stream = stream_of(ctx);
	char name[96];
	snprintf(name, sizeof(name), "rows_softmax_fwd_%s|nnc::rows::%s_softmax_fwd_kernel", sizeof(T) == 2 ? "h" : "f", row_is_wg(p.n) ? "wg" : "wave");
	note_kernel("rows_softmax_fwd");
	const double count = (double)p.rows * p.n;
	ProfScope prof(name, 6.0 * count, count * 2 * sizeof(T), p.rows, p.n, 1, 1, 1, stream);
#define ROW_CALL(NV, WG, VEC) hipLaunchKernelGGL(HIP_KERNEL_NAME(softmax_fwd_kernel<T, NV, WG, VEC>), dim3(row_grid(p.rows, p.n)), dim3(ROW_THREADS), 0, stream, p)
	ROW_FORM_DISPATCH(p.n, p.vec, ROW_CALL);
#undef ROW_CALL
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}
template <class T>
static int softmax_bwd(softmax_args_t p, ccv_nnc_stream_context_t* const ctx)
{
	if (p.rows == 0) return CCV_NNC_EXEC_SUCCESS;
	if (p.n < 1 || p.n > ROW_REG_MAX) return CCV_NNC_EXEC_INVALID;
	const void* const bases[3] = { p.g, p.b_in, p.h };
	p.vec = row_vec_ok(p.n, bases, 3);
	hipStream_t stream = stream_of(ctx);
	char name[96];
	snprintf(name, sizeof(name), "rows_softmax_bwd_%s|nnc::rows::%s_softmax_bwd_kernel", sizeof(T) == 2 ? "h" : "f", row_is_wg(p.n) ? "wg" : "wave");
	note_kernel("rows_softmax_bwd");
	const double count = (double)p.rows * p.n;
	ProfScope prof(name, 4.0 * count, count * 3 * sizeof(T), p.rows, p.n, 1, 1, 1, stream);
#define ROW_CALL(NV, WG, VEC) hipLaunchKernelGGL(HIP_KERNEL_NAME(softmax_bwd_kernel<T, NV, WG, VEC>), dim3(row_grid(p.rows, p.n)), dim3(ROW_THREADS), 0, stream, p)
	ROW_FORM_DISPATCH(p.n, p.vec, ROW_CALL);
#undef ROW_CALL
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

} // namespace rows
} // namespace nnc
