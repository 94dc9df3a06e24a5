// CMUL_FORWARD / CMUL_BACKWARD (complex multiplication of interleaved (re, im) pairs: how the reference's models apply rotary position embeddings to q and k) on
// dense CCV_16F tensors without fp32 images (cmd_detect.cpp; tunable CMUL_HALF_NATIVE), and what the fp32 command shares with them: the modes, the per-term
// expression and the broadcast geometry.
//
// Arithmetic: halves in and out, fp32 in between.  Every output element is the fp32 value cmul_kernel (cmd_detect.cpp) computes on the widened inputs -- the same
// expression (cmul_term, below), a sum that starts at +0.f and walks the reduced sub-space in the same order (axis 0 outermost) -- rounded to half ONCE on the store
// (f32_rounded, common.h): the bits of that kernel between half_up_kernel and half_down_kernel.
//
// Geometry: the fp32 kernel's argument block -- od (the output's extents), rd (what is summed per output element), per-axis strides that are 0 where an operand is
// broadcast -- general over which operand is small and on which axes.  A lane owns a VECTOR of W halves (W / 2 pairs) of the last axis, which is never broadcast:
//   W = 8   16 bytes per access: the last extent is a multiple of 8 and every base is 16-byte aligned (dense tensors: every row then is)
//   W = 2   one pair, accessed as two 2-byte elements: everything else, bases that are only 2-byte aligned included
// Two kernels:
//   cmul_half_map_kernel     nothing is summed (forward; the gradient of a full-shape operand, dq = g conj(rot)).  Laid out as the project's other maps are (DESIGN.md
//                            section 3.2, ew_map.h, bcast_ops.h): a front of workgroups over the whole tensor, 256 threads x 4 vectors each, one trip per thread, all of
//                            a lane's loads issued before its arithmetic; a vector's (i0, i1, i2) by three 32-bit divisions; the small operand's vector through its own
//                            strides (a rotary table is about 1 MB: it stays in L2)
//   cmul_half_reduce_kernel  something is summed (the gradient of a broadcast operand; CM_SUM).  One lane per OUTPUT vector walks the reduced sub-space, accumulates
//                            in fp32 and rounds once.  A long reduction is not split over lanes or workgroups: a split changes the order of the fp32 sum and with it
//                            the bits
// Index arithmetic is 32-bit: the full shape has fewer than 2^31 elements.  Bounds: a lane whose vector index is past the last one neither loads nor stores; every
// offset is a sum of (index < extent) * stride of a dense tensor, so it is inside that tensor.
// In map form the output may be the same memory as an input of its own shape: a lane reads the vectors it overwrites first, and no other lane touches them.
//
// cmul_half_plan is the ONE decision per output; cmul_half_command applies it to every requested output of a command.  half_stage.cpp's predicate
// (cmul_half_applies) and the exec functions both call it.
#pragma once
#include "chan_sums.h" // half_t

namespace nnc {

// forward   c = a * b                                               CM_MUL
// backward  g * conj(other), summed over the axes the output is 1 on   CM_MUL_CONJ
//           without g: conj(other) when nothing is broadcast        CM_CONJ
//                      the PLAIN sum of other when something is     CM_SUM   (the reference's broadcasting branch, cmul_cpu_ref.c:372-420)
enum { CM_MUL = 0, CM_MUL_CONJ = 1, CM_CONJ = 2, CM_SUM = 3 };

// one term of an output pair, in every instance of every CMUL kernel, fp32 and half
template <int MODE>
__device__ __forceinline__ void cmul_term(float& re, float& im, const float x0, const float x1, const float y0, const float y1)
{
	if (MODE == CM_CONJ) { re += x0; im += -x1; }
	else if (MODE == CM_SUM) { re += x0; im += x1; }
	else if (MODE == CM_MUL) { re += x0 * y0 - x1 * y1; im += x0 * y1 + x1 * y0; }
	else { re += x0 * y0 + x1 * y1; im += -x0 * y1 + x1 * y0; }
}

// ---- geometry (both types) -----------------------------------------------------------------------------------------------------------------------------------
struct cmul_shape4_t { int d[4]; long s[4]; };
static inline bool cmul_shape4(const ccv_nnc_tensor_t* t, cmul_shape4_t* o)
{
	const int nd = tensor_nd(t->info.dim);
	if (nd > 4 || nd < 1) return false;
	int st[CCV_NNC_MAX_DIM_ALLOC];
	tensor_strides(t, st);
	for (int k = 0; k < 4; k++) {
		const int j = k - (4 - nd);
		o->d[k] = j >= 0 ? t->info.dim[j] : 1;
		o->s[k] = (j >= 0 && o->d[k] != 1) ? st[j] : 0;
	}
	return true;
}
struct cmul_args_t { int od[4]; int rd[4]; long sx[4], sy[4], so[4]; }; // axis 3 counted in PAIRS, its strides in elements per pair
// out = reduce over the axes out is 1 on (and x / y are not) of op(x, y): the broadcast and pair-axis checks.  *full_count (where asked for): the elements of the full shape
static inline bool cmul_geometry(const ccv_nnc_tensor_t* x, const ccv_nnc_tensor_t* y, const ccv_nnc_tensor_t* out, cmul_args_t* m, double* full_count)
{
	cmul_shape4_t sx, sy, so;
	if (!cmul_shape4(x, &sx) || !cmul_shape4(out, &so) || (y && !cmul_shape4(y, &sy))) return false;
	double count = 1;
	for (int k = 0; k < 4; k++) {
		int full = sx.d[k];
		if (y && sy.d[k] > full) full = sy.d[k];
		if (so.d[k] > full) full = so.d[k];
		if ((sx.d[k] != full && sx.d[k] != 1) || (y && sy.d[k] != full && sy.d[k] != 1) || (so.d[k] != full && so.d[k] != 1)) return false;
		m->od[k] = so.d[k];
		m->rd[k] = so.d[k] == full ? 1 : full;
		m->sx[k] = sx.s[k]; m->sy[k] = y ? sy.s[k] : 0; m->so[k] = so.s[k];
		count *= full;
	}
	// the pair axis: even, dense, never broadcast (cmul_cpu_ref.c:94-95)
	if ((so.d[3] & 1) || sx.d[3] != so.d[3] || (y && sy.d[3] != so.d[3]) || so.s[3] != 1 || sx.s[3] != 1 || (y && sy.s[3] != 1)) return false;
	m->od[3] = so.d[3] / 2; m->rd[3] = 1;
	m->sx[3] = 2; m->sy[3] = 2; m->so[3] = 2;
	if (full_count) *full_count = count;
	return true;
}

// ---- the half kernels ------------------------------------------------------------------------------------------------------------------------------------------
constexpr int CMUL_THREADS = 256;
constexpr int CMUL_TILE = 4; // vectors per thread of the map kernel: a workgroup takes CMUL_TILE * CMUL_THREADS vectors

// od[3]: vectors of W halves per row; strides of axes 0 - 2 in halves (0 = broadcast); the last axis is dense in every operand
struct cmul_half_args_t { unsigned od[4], rd[3], sx[3], sy[3], so[3]; };

template <int W> struct cmul_vec { typedef half_t type __attribute__((ext_vector_type(W))); };
template <int W>
__device__ __forceinline__ typename cmul_vec<W>::type cmul_load(const half_t* const p)
{
	typedef typename cmul_vec<W>::type V;
	if constexpr (W == 2) { V v; v[0] = p[0]; v[1] = p[1]; return v; } // two 2-byte accesses: p need not be 4-byte aligned
	else return *(const V*)p;
}
template <int W>
__device__ __forceinline__ void cmul_store(half_t* const p, const typename cmul_vec<W>::type v)
{
	typedef typename cmul_vec<W>::type V;
	if constexpr (W == 2) { p[0] = v[0]; p[1] = v[1]; }
	else *(V*)p = v;
}
// the one rounding to half of every stored value
template <int W>
__device__ __forceinline__ typename cmul_vec<W>::type cmul_round(const float (&re)[W / 2], const float (&im)[W / 2])
{
	typename cmul_vec<W>::type o;
#pragma unroll
	for (int e = 0; e < W / 2; e++) { o[2 * e] = (half_t)f32_rounded(re[e]); o[2 * e + 1] = (half_t)f32_rounded(im[e]); }
	return o;
}

template <int MODE, int W>
__global__ void __launch_bounds__(CMUL_THREADS) cmul_half_map_kernel(const half_t* x, const half_t* y, half_t* out, const cmul_half_args_t m, const unsigned nv)
{
	typedef typename cmul_vec<W>::type V;
	constexpr bool HAS_Y = MODE == CM_MUL || MODE == CM_MUL_CONJ;
	const unsigned base = blockIdx.x * (CMUL_TILE * CMUL_THREADS) + threadIdx.x;
	V xv[CMUL_TILE], yv[CMUL_TILE];
	unsigned oo[CMUL_TILE];
#pragma unroll
	for (int u = 0; u < CMUL_TILE; u++) {
		const unsigned v = base + u * CMUL_THREADS;
		xv[u] = V{}; yv[u] = V{}; oo[u] = 0;
		if (v < nv) {
			unsigned r = v / m.od[3];
			const unsigned i3 = (v - r * m.od[3]) * W;
			const unsigned q = r / m.od[2], i2 = r - q * m.od[2];
			const unsigned i0 = q / m.od[1], i1 = q - i0 * m.od[1];
			oo[u] = i0 * m.so[0] + i1 * m.so[1] + i2 * m.so[2] + i3;
			xv[u] = cmul_load<W>(x + (i0 * m.sx[0] + i1 * m.sx[1] + i2 * m.sx[2] + i3));
			if (HAS_Y) yv[u] = cmul_load<W>(y + (i0 * m.sy[0] + i1 * m.sy[1] + i2 * m.sy[2] + i3));
		}
	}
#pragma unroll
	for (int u = 0; u < CMUL_TILE; u++) {
		if (base + u * CMUL_THREADS >= nv) break;
		float re[W / 2], im[W / 2];
#pragma unroll
		for (int e = 0; e < W / 2; e++) {
			re[e] = 0.f; im[e] = 0.f;
			cmul_term<MODE>(re[e], im[e], (float)xv[u][2 * e], (float)xv[u][2 * e + 1], (float)yv[u][2 * e], (float)yv[u][2 * e + 1]);
		}
		cmul_store<W>(out + oo[u], cmul_round<W>(re, im));
	}
}

template <int MODE, int W>
__global__ void __launch_bounds__(CMUL_THREADS) cmul_half_reduce_kernel(const half_t* __restrict__ x, const half_t* __restrict__ y, half_t* __restrict__ out, const cmul_half_args_t m, const unsigned nv)
{
	typedef typename cmul_vec<W>::type V;
	constexpr bool HAS_Y = MODE == CM_MUL || MODE == CM_MUL_CONJ;
	const unsigned v = blockIdx.x * CMUL_THREADS + threadIdx.x;
	if (v >= nv) return;
	const unsigned r = v / m.od[3], i3 = (v - r * m.od[3]) * W;
	const unsigned q = r / m.od[2], o2 = r - q * m.od[2];
	const unsigned o0 = q / m.od[1], o1 = q - o0 * m.od[1];
	float re[W / 2], im[W / 2];
#pragma unroll
	for (int e = 0; e < W / 2; e++) { re[e] = 0.f; im[e] = 0.f; }
	// (an axis that is summed has extent 1 in the output: o + j is j there, and o on the others)
	for (unsigned j0 = 0; j0 < m.rd[0]; j0++) for (unsigned j1 = 0; j1 < m.rd[1]; j1++) for (unsigned j2 = 0; j2 < m.rd[2]; j2++) {
		const unsigned i0 = o0 + j0, i1 = o1 + j1, i2 = o2 + j2;
		const V xv = cmul_load<W>(x + (i0 * m.sx[0] + i1 * m.sx[1] + i2 * m.sx[2] + i3));
		V yv = V{};
		if (HAS_Y) yv = cmul_load<W>(y + (i0 * m.sy[0] + i1 * m.sy[1] + i2 * m.sy[2] + i3));
#pragma unroll
		for (int e = 0; e < W / 2; e++) cmul_term<MODE>(re[e], im[e], (float)xv[2 * e], (float)xv[2 * e + 1], (float)yv[2 * e], (float)yv[2 * e + 1]);
	}
	cmul_store<W>(out + (o0 * m.so[0] + o1 * m.so[1] + o2 * m.so[2] + i3), cmul_round<W>(re, im));
}

// ---- the plan --------------------------------------------------------------------------------------------------------------------------------------------------
constexpr double CMUL_MAX_ELEMENTS = 2147483648.0; // a full shape of 2^31 elements and more keeps its route
struct cmul_half_plan_t { int mode, W, reduce; unsigned nv; cmul_half_args_t m; const half_t *x, *y; half_t* out; double bytes, pairs; };

static inline bool cmul_dense_half(const ccv_nnc_tensor_t* t) { return t && !CCV_IS_TENSOR_VIEW(t) && CCV_GET_DATA_TYPE(t->info.datatype) == CCV_16F && t->data.u8; }
// does the memory of dense tensor a meet that of dense tensor b?
static inline bool cmul_overlap(const ccv_nnc_tensor_t* a, const ccv_nnc_tensor_t* b)
{
	const uintptr_t a0 = (uintptr_t)a->data.u8, b0 = (uintptr_t)b->data.u8;
	return a0 < b0 + sizeof(half_t) * tensor_count(b->info) && b0 < a0 + sizeof(half_t) * tensor_count(a->info);
}
// true: the key is on, nothing is accumulated, x, y (where the mode has one) and out are dense CCV_16F tensors of at most four axes whose shapes pass cmul_geometry,
// the full shape has fewer than 2^31 elements, and out meets no input's memory -- except, where nothing is summed, as the same memory as an input of out's own
// shape.  *o then holds the launch (nv == 0: tensors of no elements, nothing to launch).  false: the command keeps its fp32 images.
static bool cmul_half_plan(const int mode, const ccv_nnc_tensor_t* x, const ccv_nnc_tensor_t* y, const ccv_nnc_tensor_t* out, const int flags, cmul_half_plan_t* const o)
{
	if (!tune(TUNE_CMUL_HALF_NATIVE) || (flags & CCV_NNC_ACCUMULATE_OUTPUT)) return false;
	const bool has_y = mode == CM_MUL || mode == CM_MUL_CONJ;
	if (!has_y) y = 0;
	if (!cmul_dense_half(x) || !cmul_dense_half(out) || (has_y && !cmul_dense_half(y))) return false;
	memset(o, 0, sizeof(*o));
	o->mode = mode;
	o->x = (const half_t*)x->data.u8; o->y = y ? (const half_t*)y->data.u8 : 0; o->out = (half_t*)out->data.u8;
	if (tensor_nd(x->info.dim) == 0 && tensor_nd(out->info.dim) == 0 && (!y || tensor_nd(y->info.dim) == 0)) return true; // no elements
	cmul_args_t g;
	double full;
	if (!cmul_geometry(x, y, out, &g, &full) || full >= CMUL_MAX_ELEMENTS) return false;
	o->reduce = g.rd[0] > 1 || g.rd[1] > 1 || g.rd[2] > 1;
	for (int k = 0; k < 2; k++) {
		const ccv_nnc_tensor_t* const in = k ? y : x;
		if (!in || !cmul_overlap(in, out)) continue;
		if (o->reduce || in->data.u8 != out->data.u8 || tensor_count(in->info) != tensor_count(out->info)) return false; // (the same count under cmul_geometry: the same shape)
	}
	const int last = g.od[3] * 2;
	o->W = last % 8 == 0 && aligned16(o->x) && aligned16(o->out) && (!y || aligned16(o->y)) ? 8 : 2;
	cmul_half_args_t& m = o->m;
	for (int k = 0; k < 3; k++) { m.od[k] = (unsigned)g.od[k]; m.rd[k] = (unsigned)g.rd[k]; m.sx[k] = (unsigned)g.sx[k]; m.sy[k] = (unsigned)g.sy[k]; m.so[k] = (unsigned)g.so[k]; }
	m.od[3] = (unsigned)(last / o->W);
	o->nv = m.od[0] * m.od[1] * m.od[2] * m.od[3];
	o->pairs = full / 2;
	o->bytes = sizeof(half_t) * ((double)tensor_count(x->info) + (y ? (double)tensor_count(y->info) : 0.) + (double)tensor_count(out->info));
	return true;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------------------------
template <int MODE, int W>
static void cmul_half_launch(const cmul_half_plan_t& p, hipStream_t stream)
{
	if (p.reduce) hipLaunchKernelGGL(HIP_KERNEL_NAME(cmul_half_reduce_kernel<MODE, W>), dim3((p.nv + CMUL_THREADS - 1) / CMUL_THREADS), dim3(CMUL_THREADS), 0, stream, p.x, p.y, p.out, p.m, p.nv);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(cmul_half_map_kernel<MODE, W>), dim3((p.nv + CMUL_TILE * CMUL_THREADS - 1) / (CMUL_TILE * CMUL_THREADS)), dim3(CMUL_THREADS), 0, stream, p.x, p.y, p.out, p.m, p.nv);
}
template <int MODE>
static void cmul_half_launch_w(const cmul_half_plan_t& p, hipStream_t stream)
{
	if (p.W == 8) cmul_half_launch<MODE, 8>(p, stream);
	else cmul_half_launch<MODE, 2>(p, stream);
}
// one launch; the record: "<row>|nnc::cmul_half_map_kernel<MODE,W>" / "...cmul_half_reduce_kernel<MODE,W>"
static int cmul_half_run(const char* row, const cmul_half_plan_t& p, ccv_nnc_stream_context_t* ctx)
{
	if (p.nv == 0) return CCV_NNC_EXEC_SUCCESS;
	static const char* const modes[4] = { "MUL", "MUL_CONJ", "CONJ", "SUM" };
	hipStream_t stream = stream_of(ctx);
	char name[96];
	snprintf(name, sizeof(name), "%s|nnc::cmul_half_%s_kernel<%s,%d>", row, p.reduce ? "reduce" : "map", modes[p.mode], p.W);
	note_kernel(p.reduce ? "cmul_half_reduce" : "cmul_half_map");
	ProfScope prof(name, (p.mode == CM_MUL || p.mode == CM_MUL_CONJ ? 6. : 2.) * p.pairs, p.bytes, (int)p.m.od[0], (int)p.m.od[1], (int)p.m.od[2], (int)(p.m.od[3] * p.W), 1, stream);
	switch (p.mode) {
		case CM_MUL: cmul_half_launch_w<CM_MUL>(p, stream); break;
		case CM_MUL_CONJ: cmul_half_launch_w<CM_MUL_CONJ>(p, stream); break;
		case CM_CONJ: cmul_half_launch_w<CM_CONJ>(p, stream); break;
		default: cmul_half_launch_w<CM_SUM>(p, stream); break;
	}
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

} // namespace nnc
