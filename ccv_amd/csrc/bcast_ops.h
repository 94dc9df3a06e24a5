// Broadcast arithmetic on dense CCV_16F tensors without fp32 images: ADD, same-shape MUL, SCALAR_MUL, REDUCE_SUM and REDUCE_MEAN, forward and backward
// (cmd_bcast.cpp, cmd_ew.cpp; tunable BCAST_HALF_NATIVE).  Halves in and out, fp32 arithmetic, every output rounded once from the fp32 value of its expression
// (f32_rounded, common.h: the bits of the fp32 kernel followed by a conversion); sums accumulate in fp32 and are rounded once at the end.
//
// Geometry (bcast_geom): the shapes right-aligned to four axes, one tensor ("big") of the full shape, the other ("small") with big's extent or 1 on every axis.
// Axes on which big's extent is 1 are dropped, neighbours of one kind (kept / broadcast) merged; what remains is
//   flat     nothing is broadcast                                                      ew_map_kernel (ew_map.h) with the functors below
//   period   big [I][R][Cc], small [I][Cc]       bias [..., C] + [C], NHWC maps        bcast_period_kernel; sums: chan_reduce_rows (I == 1), rows_image_sum (I <= 65535)
//   run      big [Q][M][L],  small [M]           NCHW maps against [1,C,1,1] / [N,C,1,1], [A][B] against [A][1], a one-element small (Q = M = 1)
//                                                                                      bcast_run_kernel; sums: chan_reduce_planes_sliced
// or four alternating groups, which are refused (the command keeps the generic kernels on fp32 images), as is everything with 2^31 elements or more.
// The maps are laid out over the whole tensor, a front of workgroups with one trip per thread; the sums are chan_sums.h's two
// deterministic stages.  An output may be the same tensor as a same-shape input: every lane reads what it overwrites first.
// bcast_half_plan is the ONE decision: half_stage.cpp's predicate (bcast_half_applies) and the exec functions (bcast_half_exec) both call it.
#pragma once
#include "ew_map.h"

namespace nnc {

constexpr int BC_THREADS = 256, BC_TILE = 4; // a workgroup takes 4 x 256 vectors (or elements), as the element-wise maps do

// ---- functors ----------------------------------------------------------------------------------------------------------------------------------------
// flat (ew_map_kernel's three-operand form)
struct BScale { float p; __device__ float operator()(float a, float, float) const { return f32_rounded(p * a); } };
struct BAxpby { float p, q; __device__ float operator()(float a, float b, float) const { return f32_rounded(p * a + q * b); } };
struct BMul { float p; __device__ float operator()(float a, float b, float) const { return f32_rounded((p * a) * b); } }; // FMul's operand order
// broadcast (x of the big tensor, s of the small one); `first`: the small tensor is the command's first operand
struct BcAdd { float p, q; int first; __device__ float operator()(float x, float s) const { return f32_rounded(first ? p * s + q * x : p * x + q * s); } };
struct BcScale { float p; __device__ float operator()(float, float s) const { return f32_rounded(p * s); } }; // a gradient broadcast back: no big operand

// ---- kernels -----------------------------------------------------------------------------------------------------------------------------------------
// period: out[i][r][c] = f(big[i][r][c], small[i][c]).  W = 8: 16-byte lanes along Cc (Cc % 8 == 0, every base 16-byte aligned), W = 1 otherwise; cv = Cc / W lanes
// per row.  A workgroup is cvt column lanes (a power of two) x 256 / cvt row phases and takes BC_TILE rows per phase: a lane loads its small vector once and
// reuses it down its rows.  Rows wider than 256 lanes take several column tiles.  blockIdx.x = ((image * chunks) + row chunk) * tiles + column tile.
template <class F, bool HAS_BIG, int W>
__global__ void __launch_bounds__(BC_THREADS) bcast_period_kernel(F f, const half_t* big, const half_t* small, half_t* out, const unsigned R, const unsigned cv, const int cvt_log2, const unsigned tiles, const unsigned chunks)
{
	typedef half_t V __attribute__((ext_vector_type(W)));
	const unsigned cvt = 1u << cvt_log2, q = threadIdx.x & (cvt - 1), phase = threadIdx.x >> cvt_log2, phases = BC_THREADS >> cvt_log2;
	unsigned b = blockIdx.x;
	const unsigned tile = b % tiles;
	b /= tiles;
	const unsigned chunk = b % chunks, i = b / chunks;
	const unsigned c = tile * cvt + q;
	if (c >= cv) return;
	const V s = ((const V*)small)[(size_t)i * cv + c];
	const unsigned r0 = chunk * (phases * BC_TILE) + phase;
	const size_t base = (size_t)i * R * cv + c;
	V x[BC_TILE];
#pragma unroll
	for (int u = 0; u < BC_TILE; u++) {
		const unsigned r = r0 + u * phases;
		x[u] = HAS_BIG && r < R ? ((const V*)big)[base + (size_t)r * cv] : V{};
	}
#pragma unroll
	for (int u = 0; u < BC_TILE; u++) {
		const unsigned r = r0 + u * phases;
		if (r >= R) break;
		V o;
#pragma unroll
		for (int e = 0; e < W; e++) o[e] = (half_t)f((float)x[u][e], (float)s[e]);
		((V*)out)[base + (size_t)r * cv] = o;
	}
}

// run: out[e] = f(big[e], small[(e / L) % M]), one small value per run of L contiguous elements.  The work is laid out over ELEMENTS, not runs: one run of the
// whole tensor and runs of two elements fill the chip alike.  W = 8: a lane takes 16-byte vectors of the flat tensor (big and out 16-byte aligned); a vector
// inside one run broadcasts one small value, one that straddles runs (L = 35: every run from the second on starts unaligned) walks them.  W = 1: an element per
// lane.  nv whole vectors; the last n - nv * W elements go to the first lanes of workgroup 0.
template <class F, bool HAS_BIG, int W>
__global__ void __launch_bounds__(BC_THREADS) bcast_run_kernel(F f, const half_t* big, const half_t* small, half_t* out, const unsigned L, const unsigned M, const unsigned nv, const unsigned n)
{
	typedef half_t V __attribute__((ext_vector_type(W)));
	const unsigned base = blockIdx.x * (BC_TILE * BC_THREADS) + threadIdx.x;
	V x[BC_TILE];
#pragma unroll
	for (int u = 0; u < BC_TILE; u++) {
		const unsigned v = base + u * BC_THREADS;
		x[u] = HAS_BIG && v < nv ? ((const V*)big)[v] : V{};
	}
#pragma unroll
	for (int u = 0; u < BC_TILE; u++) {
		const unsigned v = base + u * BC_THREADS;
		if (v >= nv) break;
		const unsigned e0 = v * W, run = e0 / L;
		unsigned r = e0 - run * L, m = run % M;
		V o;
		if (W == 1 || r + W <= L) { // the whole vector inside one run
			const float s = (float)small[m];
#pragma unroll
			for (int e = 0; e < W; e++) o[e] = (half_t)f((float)x[u][e], s);
		} else {
#pragma unroll
			for (int e = 0; e < W; e++) {
				o[e] = (half_t)f((float)x[u][e], (float)small[m]);
				if (++r == L) { r = 0; if (++m == M) m = 0; }
			}
		}
		((V*)out)[v] = o;
	}
	const unsigned t = nv * W + threadIdx.x;
	if (blockIdx.x == 0 && t < n) out[t] = (half_t)f(HAS_BIG ? (float)big[t] : 0.f, (float)small[(t / L) % M]);
}

// ---- geometry ----------------------------------------------------------------------------------------------------------------------------------------
enum { BC_FLAT = 1, BC_PERIOD = 2, BC_RUN = 3 };
struct bcast_geom_t { int form; unsigned n, I, R, Cc, Q, M, L; }; // n: big's elements (< 2^31)
constexpr unsigned BC_MAX_IMAGES = 65535; // SUMS in period form with I > 1: the images are a grid dimension of rows_image_sum (bc_sum_geom; the maps have no such limit)

// dims right-aligned to four axes, as cmd_bcast.cpp's shape4() does
static inline bool bcast_dims4(const ccv_nnc_tensor_t* t, int d[4])
{
	const int nd = tensor_nd(t->info.dim);
	if (nd > 4) return false;
	for (int k = 0; k < 4; k++) { const int j = k - (4 - nd); d[k] = j >= 0 ? t->info.dim[j] : 1; }
	return true;
}
static inline bool bcast_geom(const int big[4], const int small[4], bcast_geom_t* o)
{
	unsigned g[4] = { 0, 0, 0, 0 };
	int kept[4], ng = 0;
	double n = 1;
	for (int k = 0; k < 4; k++) {
		if (big[k] < 1 || (small[k] != big[k] && small[k] != 1)) return false;
		if (big[k] == 1) continue;
		const int kd = small[k] == big[k];
		n *= big[k];
		if (n >= 2147483648.0) return false;
		if (ng && kept[ng - 1] == kd) g[ng - 1] *= (unsigned)big[k];
		else { g[ng] = (unsigned)big[k]; kept[ng++] = kd; }
	}
	memset(o, 0, sizeof(*o));
	o->n = (unsigned)n;
	if (ng == 0 || (ng == 1 && kept[0])) { o->form = BC_FLAT; return true; }
	if (ng == 1) { o->form = BC_RUN; o->Q = 1; o->M = 1; o->L = g[0]; return true; }
	if (ng == 2 && kept[0]) { o->form = BC_RUN; o->Q = 1; o->M = g[0]; o->L = g[1]; return true; }
	if (ng == 2) { o->form = BC_PERIOD; o->I = 1; o->R = g[0]; o->Cc = g[1]; return true; }
	if (ng == 3 && kept[0]) { o->form = BC_PERIOD; o->I = g[0]; o->R = g[1]; o->Cc = g[2]; return true; }
	if (ng == 3) { o->form = BC_RUN; o->Q = g[0]; o->M = g[1]; o->L = g[2]; return true; }
	return false; // four alternating groups
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------------------------
// A command is one or two operations on raw pointers.  MAP: out = fn(x[, y]) over n elements.  BCAST: out (big's shape) = fn(big, small).  SUM: out (small) = p * the
// sum of big over what was broadcast.
enum { BOP_MAP = 1, BOP_BCAST = 2, BOP_SUM = 3 };
enum { BFN_SCALE = 1, BFN_AXPBY = 2, BFN_MUL = 3 };
struct bcast_op_t { int kind, fn, first; bcast_geom_t g; const half_t *x, *y; half_t* out; float p, q; };
struct bcast_plan_t { int nops; const char* tag; bcast_op_t op[2]; };

static inline bool bc_half(const ccv_nnc_tensor_t* t, int d[4]) { return t && !CCV_IS_TENSOR_VIEW(t) && CCV_GET_DATA_TYPE(t->info.datatype) == CCV_16F && bcast_dims4(t, d); }
static inline bool bc_same(const int a[4], const int b[4]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }
static inline bcast_op_t* bc_op(bcast_plan_t* o, const int kind, const int fn, const ccv_nnc_tensor_t* x, const ccv_nnc_tensor_t* y, ccv_nnc_tensor_t* out, const float p, const float q)
{
	bcast_op_t* const op = &o->op[o->nops++];
	op->kind = kind; op->fn = fn; op->first = 0; op->x = x ? (const half_t*)x->data.u8 : 0; op->y = y ? (const half_t*)y->data.u8 : 0; op->out = (half_t*)out->data.u8; op->p = p; op->q = q;
	return op;
}
static inline bool bc_sum_geom(const int big[4], const int small[4], bcast_geom_t* g) { return bcast_geom(big, small, g) && g->form != BC_FLAT && (g->form != BC_PERIOD || g->I <= BC_MAX_IMAGES); }
static inline bool bc_flat(bcast_plan_t* o, const int fn, const ccv_nnc_tensor_t* x, const ccv_nnc_tensor_t* y, ccv_nnc_tensor_t* out, const int d[4], const float p, const float q)
{
	bcast_op_t* const op = bc_op(o, BOP_MAP, fn, x, y, out, p, q);
	return bcast_geom(d, d, &op->g); // (false: no elements, or 2^31 and more)
}
// true: every tensor the command uses is a dense CCV_16F tensor of at most four dimensions, nothing is accumulated, g is there for the backward commands and
// the shapes are flat, a period or runs -- *o then holds the operations.  false: the command keeps today's route.
static bool bcast_half_plan(const ccv_nnc_cmd_t cmd, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, bcast_plan_t* const o)
{
	if (!tune(TUNE_BCAST_HALF_NATIVE) || (flags & CCV_NNC_ACCUMULATE_OUTPUT)) return false;
	memset(o, 0, sizeof(*o));
	const ccv_nnc_tensor_t* const i0 = input_size > 0 ? inputs[0] : 0;
	const ccv_nnc_tensor_t* const i1 = input_size > 1 ? inputs[1] : 0;
	const ccv_nnc_tensor_t* const i2 = input_size > 2 ? inputs[2] : 0;
	ccv_nnc_tensor_t* const o0 = output_size > 0 ? outputs[0] : 0;
	ccv_nnc_tensor_t* const o1 = output_size > 1 ? outputs[1] : 0;
	int d0[4], d1[4], d2[4], e[4];
	if (!bc_half(i0, d0)) return false; // (a or g: every command here has it)
	switch (cmd.cmd) {
		case CCV_NNC_SCALAR_MUL_FORWARD:
		case CCV_NNC_SCALAR_MUL_BACKWARD:
			o->tag = "scalar_mul";
			return bc_half(o0, e) && tensor_count(i0->info) == tensor_count(o0->info) && bc_flat(o, BFN_SCALE, i0, 0, o0, e, cmd.info.blas.a[0], 0.f);
		case CCV_NNC_ADD_FORWARD: {
			o->tag = "add_fwd";
			const float p = cmd.info.blas.a[0], q = cmd.info.blas.a[1];
			if (!bc_half(o0, e)) return false;
			if (!i1) return bc_same(d0, e) && bc_flat(o, BFN_SCALE, i0, 0, o0, e, p, 0.f);
			if (!bc_half(i1, d1)) return false;
			const bool a_full = bc_same(d0, e), b_full = bc_same(d1, e);
			if (a_full && b_full) return bc_flat(o, BFN_AXPBY, i0, i1, o0, e, p, q);
			if (!a_full && !b_full) return false; // neither operand has the output's shape
			bcast_op_t* const op = bc_op(o, BOP_BCAST, BFN_AXPBY, a_full ? i0 : i1, a_full ? i1 : i0, o0, p, q);
			op->first = !a_full;
			return bcast_geom(e, a_full ? d1 : d0, &op->g) && op->g.form != BC_FLAT;
		}
		case CCV_NNC_ADD_BACKWARD: { // g -> da = p g, db = q g, each summed over what it was broadcast along
			o->tag = "add_bwd";
			if (!o0 && !o1) return false;
			for (int k = 0; k < 2; k++) {
				ccv_nnc_tensor_t* const t = k ? o1 : o0;
				if (!t) continue;
				if (!bc_half(t, e)) return false;
				if (bc_same(d0, e)) { if (!bc_flat(o, BFN_SCALE, i0, 0, t, e, cmd.info.blas.a[k], 0.f)) return false; continue; }
				bcast_op_t* const op = bc_op(o, BOP_SUM, BFN_SCALE, i0, 0, t, cmd.info.blas.a[k], 0.f);
				if (!bc_sum_geom(d0, e, &op->g)) return false;
			}
			return true;
		}
		case CCV_NNC_MUL_FORWARD: // flat only: a broadcast operand keeps mul_planes.h or the fp32 images
			o->tag = "mul_fwd";
			return bc_half(i1, d1) && bc_half(o0, e) && bc_same(d0, e) && bc_same(d1, e) && bc_flat(o, BFN_MUL, i0, i1, o0, e, cmd.info.blas.a[0], 0.f);
		case CCV_NNC_MUL_BACKWARD: // g, a, b -> da = (p g) b, db = (p g) a
			o->tag = "mul_bwd";
			if ((!o0 && !o1) || !bc_half(i1, d1) || !bc_half(i2, d2) || !bc_same(d0, d1) || !bc_same(d0, d2)) return false;
			if (o0 && (!bc_half(o0, e) || !bc_same(d0, e) || !bc_flat(o, BFN_MUL, i0, i2, o0, e, cmd.info.blas.a[0], 0.f))) return false;
			if (o1 && (!bc_half(o1, e) || !bc_same(d0, e) || !bc_flat(o, BFN_MUL, i0, i1, o1, e, cmd.info.blas.a[0], 0.f))) return false;
			return true;
		case CCV_NNC_REDUCE_SUM_FORWARD:
		case CCV_NNC_REDUCE_MEAN_FORWARD: {
			o->tag = "reduce_fwd";
			if (!bc_half(o0, e)) return false;
			if (bc_same(d0, e)) return bc_flat(o, BFN_SCALE, i0, 0, o0, e, 1.f, 0.f); // nothing is reduced
			const size_t no = tensor_count(o0->info);
			const float p = cmd.cmd == CCV_NNC_REDUCE_MEAN_FORWARD && no ? 1.f / (float)(tensor_count(i0->info) / no) : 1.f;
			bcast_op_t* const op = bc_op(o, BOP_SUM, BFN_SCALE, i0, 0, o0, p, 0.f);
			return bc_sum_geom(d0, e, &op->g);
		}
		case CCV_NNC_REDUCE_SUM_BACKWARD:
		case CCV_NNC_REDUCE_MEAN_BACKWARD: { // h = g (times 1 / count) broadcast back
			o->tag = "reduce_bwd";
			if (!bc_half(o0, e)) return false;
			const size_t ng = tensor_count(i0->info);
			const float p = cmd.cmd == CCV_NNC_REDUCE_MEAN_BACKWARD ? 1.f / (float)(tensor_count(o0->info) / (ng ? ng : 1)) : 1.f;
			if (bc_same(d0, e)) return bc_flat(o, BFN_SCALE, i0, 0, o0, e, p, 0.f);
			bcast_op_t* const op = bc_op(o, BOP_BCAST, BFN_SCALE, 0, i0, o0, p, 0.f);
			return bcast_geom(e, d0, &op->g) && op->g.form != BC_FLAT;
		}
	}
	return false;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------------------
// the launch record: "bcast_<command>|nnc::<kernel>" (ProfScope copies it; note_kernel keeps the pointer it is given, so it gets literals: bcast_flat / _period / _run / _sum)
struct bcast_prof_name_t { char s[96]; bcast_prof_name_t(const char* tag, const char* kernel) { snprintf(s, sizeof(s), "bcast_%s|nnc::%s", tag, kernel); } };

template <class F, bool HAS_BIG>
static int bcast_period_map(const char* tag, F f, const bcast_geom_t& g, const half_t* big, const half_t* small, half_t* out, ccv_nnc_stream_context_t* ctx)
{
	const bool vec = g.Cc % 8 == 0 && aligned16(out) && aligned16(small) && (!HAS_BIG || aligned16(big));
	const unsigned cv = vec ? g.Cc / 8 : g.Cc;
	int l = 0;
	while ((1u << l) < cv && (1 << l) < BC_THREADS) l++;
	const unsigned cvt = 1u << l, rows = (BC_THREADS >> l) * BC_TILE, tiles = (cv + cvt - 1) / cvt, chunks = (g.R + rows - 1) / rows;
	const size_t blocks = (size_t)g.I * chunks * tiles; // <= n < 2^31
	hipStream_t stream = stream_of(ctx);
	const bcast_prof_name_t name(tag, "bcast_period_kernel");
	note_kernel("bcast_period");
	ProfScope prof(name.s, (double)g.n, sizeof(half_t) * ((HAS_BIG ? 2.0 : 1.0) * (double)g.n + (double)g.I * g.Cc), (int)g.I, (int)g.R, (int)g.Cc, 1, 1, stream);
	if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(bcast_period_kernel<F, HAS_BIG, 8>), dim3((unsigned)blocks), dim3(BC_THREADS), 0, stream, f, big, small, out, g.R, cv, l, tiles, chunks);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(bcast_period_kernel<F, HAS_BIG, 1>), dim3((unsigned)blocks), dim3(BC_THREADS), 0, stream, f, big, small, out, g.R, cv, l, tiles, chunks);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}
template <class F, bool HAS_BIG>
static int bcast_run_map(const char* tag, F f, const bcast_geom_t& g, const half_t* big, const half_t* small, half_t* out, ccv_nnc_stream_context_t* ctx)
{
	const bool vec = aligned16(out) && (!HAS_BIG || aligned16(big));
	const unsigned nv = vec ? g.n / 8 : g.n;
	const unsigned blocks = nv ? (nv + BC_TILE * BC_THREADS - 1) / (BC_TILE * BC_THREADS) : 1;
	hipStream_t stream = stream_of(ctx);
	const bcast_prof_name_t name(tag, "bcast_run_kernel");
	note_kernel("bcast_run");
	ProfScope prof(name.s, (double)g.n, sizeof(half_t) * ((HAS_BIG ? 2.0 : 1.0) * (double)g.n + (double)g.M), (int)g.Q, (int)g.M, (int)g.L, 1, 1, stream);
	if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(bcast_run_kernel<F, HAS_BIG, 8>), dim3(blocks), dim3(BC_THREADS), 0, stream, f, big, small, out, g.L, g.M, nv, g.n);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(bcast_run_kernel<F, HAS_BIG, 1>), dim3(blocks), dim3(BC_THREADS), 0, stream, f, big, small, out, g.L, g.M, nv, g.n);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}
template <class F, bool HAS_BIG>
static int bcast_half_map(const char* tag, F f, const bcast_op_t& op, ccv_nnc_stream_context_t* ctx)
{
	if (op.g.form == BC_PERIOD) return bcast_period_map<F, HAS_BIG>(tag, f, op.g, op.x, op.y, op.out, ctx);
	return bcast_run_map<F, HAS_BIG>(tag, f, op.g, op.x, op.y, op.out, ctx);
}
template <class F, int NIN>
static int bcast_half_flat(const char* tag, F f, const bcast_op_t& op, ccv_nnc_stream_context_t* ctx)
{
	hipStream_t stream = stream_of(ctx);
	const bcast_prof_name_t name(tag, "ew_map_kernel");
	note_kernel("bcast_flat");
	ProfScope prof(name.s, (double)op.g.n, sizeof(half_t) * (NIN + 1.0) * (double)op.g.n, (int)op.g.n, 1, 1, 1, 1, stream);
	return ew_map<F, NIN, half_t>(f, op.out, op.x, op.y, (const half_t*)0, op.g.n, ctx);
}
// out (small) = the sum of p x over what was broadcast: fp32 partials in the stream workspace, a fixed-order fold that rounds once (chan_sums.h)
static int bcast_half_sum(const char* tag, const bcast_op_t& op, ccv_nnc_stream_context_t* ctx)
{
	const bcast_geom_t& g = op.g;
	RScaled f;
	f.s = op.p;
	hipStream_t stream = stream_of(ctx);
	const chan_view_t v = { (long)g.Q, (int)g.M, (long)g.L };
	const bcast_prof_name_t name(tag, g.form == BC_RUN ? chan_planes_kernel_name(v) : g.I == 1 ? "chan_reduce_rows_kernel" : "rows_image_sum_kernel"); // (the first of the two launches; chan_fold_kernel follows)
	note_kernel("bcast_sum");
	ProfScope prof(name.s, (double)g.n, sizeof(half_t) * (double)g.n, (int)(g.form == BC_RUN ? g.Q : g.I), (int)(g.form == BC_RUN ? g.M : g.R), (int)(g.form == BC_RUN ? g.L : g.Cc), 1, 1, stream);
	if (g.form == BC_PERIOD) {
		if (g.I == 1) return chan_reduce_rows<RScaled, false, half_t, half_t>(f, op.x, (const half_t*)0, (long)g.R, (int)g.Cc, (long)g.Cc, op.out, 0, ctx);
		return rows_image_sum<RScaled, half_t, half_t>(f, op.x, (int)g.I, (long)g.R, (int)g.Cc, op.out, ctx);
	}
	return chan_reduce_planes_sliced<RScaled, false, half_t, half_t>(f, op.x, (const half_t*)0, v, op.out, 0, ctx);
}
static int bcast_half_run(const bcast_plan_t& bp, ccv_nnc_stream_context_t* ctx)
{
	for (int k = 0; k < bp.nops; k++) {
		const bcast_op_t& op = bp.op[k];
		int ret = CCV_NNC_EXEC_INVALID;
		if (op.kind == BOP_SUM) ret = bcast_half_sum(bp.tag, op, ctx);
		else if (op.kind == BOP_MAP) {
			if (op.fn == BFN_SCALE) { BScale f; f.p = op.p; ret = bcast_half_flat<BScale, 1>(bp.tag, f, op, ctx); }
			else if (op.fn == BFN_AXPBY) { BAxpby f; f.p = op.p; f.q = op.q; ret = bcast_half_flat<BAxpby, 2>(bp.tag, f, op, ctx); }
			else { BMul f; f.p = op.p; ret = bcast_half_flat<BMul, 2>(bp.tag, f, op, ctx); }
		} else if (op.fn == BFN_AXPBY) { BcAdd f; f.p = op.p; f.q = op.q; f.first = op.first; ret = bcast_half_map<BcAdd, true>(bp.tag, f, op, ctx); }
		else { BcScale f; f.p = op.p; ret = bcast_half_map<BcScale, false>(bp.tag, f, op, ctx); }
		if (ret != CCV_NNC_EXEC_SUCCESS) return ret;
	}
	return CCV_NNC_EXEC_SUCCESS;
}

} // namespace nnc
