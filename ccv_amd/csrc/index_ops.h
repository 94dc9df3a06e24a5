// INDEX_SELECT_FORWARD / BACKWARD (embedding gather, ordered scatter-add) and PAD_FORWARD / BACKWARD on dense CCV_16F tensors without fp32 images
// (cmd_index_pad.cpp; tunable INDEX_PAD_HALF_NATIVE), the ordered scatter-add of the fp32 command on the same kernel (tunable INDEX_BACK_TILES), and the
// interpolation expression and the pad kernels the fp32 commands share with them.
//
// Arithmetic: halves in and out, fp32 in between, ONE rounding to half on the store (f32_rounded, common.h).
//   gather        int32 indices: a copy of rows.  fp32 indices: index_lerp on the widened values -- the expression of the fp32 kernel, in the same function.
//   scatter-add   for every (destination row, column) the sum starts at +0.f, adds the sources in ascending source-row order in fp32 and is stored once:
//                 the bits of index_scatter_add_kernel after zero_rows_kernel, and of that pair between half_up_kernel and half_down_kernel.  Nothing is
//                 accumulated in half, there is no fp32 image of the table, there are no floating-point atomics.  Rows no index names are written as zeros by
//                 the same kernel: no zeroing pass.
//   pad           a copy; zero fill is +0.
//
// The scatter-add.  A tile is IDX_TILE_ROWS consecutive destination rows by IDX_THREADS * VEC columns, owned by ONE wave; its fp32 accumulators live in LDS
// (IDX_TILE_ROWS * VEC * IDX_THREADS * 4 bytes: 16 KB for halves, 8 KB for fp32 -- ten / twenty tiles to a CU's 160 KB).  A lane owns VEC adjacent columns, so
// the read-modify-writes of one accumulator are one lane's, in program order: ordered by construction, no barrier anywhere in the kernel.  The wave finds its
// sources itself: it reads the indices IDX_CHUNK at a time (four coalesced loads of 64), compares each with its row range, and __ballot gives it the sources
// of the chunk that are its own as four masks, which it walks from the lowest bit up -- ascending source row.  Up to IDX_AHEAD source rows are loaded before
// the first of them is added, so a row many indices name costs a fraction of a memory latency per source, not a whole one.
// Nothing is counted, listed or read back by the host: no workspace, every grid depends on shapes alone, the command is capturable as it stands.
// (Per-tile source lists from a stable bucket pass over the indices -- count, scan, fill -- would spare the tiles the scan of indices that are not theirs, at three
// more launches and a workspace of tiles * chunks counters; they are not built here)
// Bounds: an index outside [0, rows of h) matches no tile (or a row of the last tile that is never stored) and is ignored; loads of g are of sources
// s < g_rows only; stores are of rows < h_rows and of columns < cols only (VEC > 1: cols % VEC == 0, so a lane's columns are inside together).
//
// index_half_plan / index_back_plan / pad_half_plan are the ONE decision each: half_stage.cpp's predicate (index_pad_half_applies) and the exec functions call them.
#pragma once
#include "chan_sums.h" // half_t

namespace nnc {

// ---- the fp32-index interpolation (index_select_cpu_ref.c:49-60) -------------------------------------------------------------------------------------
struct IdxLerp { int j0, j1; float w0, w1; };
__device__ __forceinline__ IdxLerp index_lerp_rows(const float f, const int a_rows)
{
	IdxLerp c;
	c.j0 = (int)f;
	c.j1 = c.j0 + 1 < a_rows - 1 ? c.j0 + 1 : a_rows - 1;
	c.w1 = f - c.j0;
	c.w0 = 1.f - c.w1;
	return c;
}
__device__ __forceinline__ float index_lerp(const float a0, const float a1, const IdxLerp& c) { return a0 * c.w0 + a1 * c.w1; }

// ---- gather ------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int IDX_GATHER_THREADS = 256;
template <typename T> struct idx_widen { static __device__ __forceinline__ T round(const float v) { return (T)f32_rounded(v); } }; // the one rounding to half
template <> struct idx_widen<float> { static __device__ __forceinline__ float round(const float v) { return v; } };
template <typename I> struct idx_is_f32 { enum { value = 0 }; };
template <> struct idx_is_f32<float> { enum { value = 1 }; };

// b[r][:] = a[idx[r]][:] (I = int), or the interpolation between rows (int)idx[r] and the next (I = float).  A wave per row of b, rows dealt over the waves of the
// grid; idx[r] is read once per row and is wave-uniform.  VEC = 8: cols % 8 == 0, both bases 16-byte aligned, so every row is.
template <typename T, int VEC, typename I>
__global__ void __launch_bounds__(IDX_GATHER_THREADS) index_gather_kernel(const T* __restrict__ a, const I* __restrict__ idx, T* __restrict__ b, const int rows, const int cols, const int a_rows)
{
	typedef T V __attribute__((ext_vector_type(VEC)));
	const unsigned lane = threadIdx.x & 63, waves = blockDim.x >> 6, cv = (unsigned)cols / VEC;
	for (unsigned r = blockIdx.x * waves + (threadIdx.x >> 6); r < (unsigned)rows; r += gridDim.x * waves) {
		V* const dst = (V*)(b + (size_t)r * cols);
		if (!idx_is_f32<I>::value) {
			const V* const src = (const V*)(a + (size_t)(long)idx[r] * cols);
			for (unsigned c = lane; c < cv; c += 64) dst[c] = src[c];
		} else {
			const IdxLerp k = index_lerp_rows((float)idx[r], a_rows);
			const V* const s0 = (const V*)(a + (size_t)k.j0 * cols);
			const V* const s1 = (const V*)(a + (size_t)k.j1 * cols);
			for (unsigned c = lane; c < cv; c += 64) {
				const V v0 = s0[c], v1 = s1[c];
				V o;
#pragma unroll
				for (int e = 0; e < VEC; e++) o[e] = idx_widen<T>::round(index_lerp((float)v0[e], (float)v1[e], k));
				dst[c] = o;
			}
		}
	}
}

// ---- ordered scatter-add ---------------------------------------------------------------------------------------------------------------------------------
constexpr int IDX_THREADS = 64;   // one wave per tile
constexpr int IDX_TILE_ROWS = 8;  // destination rows of a tile
constexpr int IDX_CHUNK = 256;    // indices a wave examines per step: four per lane
constexpr int IDX_AHEAD = 4;      // source rows loaded before the first of them is added

template <typename T, int VEC>
__global__ void __launch_bounds__(IDX_THREADS) index_scatter_tile_kernel(const T* __restrict__ g, const int* __restrict__ idx, T* __restrict__ h, const int g_rows, const int h_rows, const int cols, const unsigned col_chunks, const unsigned tiles)
{
	typedef T V __attribute__((ext_vector_type(VEC)));
	__shared__ float acc[IDX_TILE_ROWS][VEC][IDX_THREADS]; // [row][element][lane]: a lane's accesses are its own words, neighbouring lanes on neighbouring banks
	const int lane = threadIdx.x;
	for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
		const unsigned rt = tile / col_chunks, cc = tile - rt * col_chunks;
		const unsigned row0 = rt * IDX_TILE_ROWS;
		const unsigned col = (cc * IDX_THREADS + lane) * VEC;
		const bool live = col < (unsigned)cols; // (every lane stays for the ballots)
#pragma unroll
		for (int r = 0; r < IDX_TILE_ROWS; r++)
#pragma unroll
			for (int e = 0; e < VEC; e++) acc[r][e][lane] = 0.f;
		for (unsigned base = 0; base < (unsigned)g_rows; base += IDX_CHUNK) { // (unsigned: g_rows < 2^31, so base + IDX_CHUNK does not wrap)
			unsigned long long m[IDX_CHUNK / 64];
#pragma unroll
			for (int k = 0; k < IDX_CHUNK / 64; k++) {
				const unsigned s = base + 64 * k + lane;
				const unsigned r = s < (unsigned)g_rows ? (unsigned)idx[s] - row0 : ~0u;
				m[k] = __ballot(r < (unsigned)IDX_TILE_ROWS);
			}
#pragma unroll
			for (int k = 0; k < IDX_CHUNK / 64; k++) {
				unsigned long long mk = m[k]; // wave-uniform: the walk below is the same in every lane
				while (mk) {
					unsigned s[IDX_AHEAD];
					int n = 0;
					V v[IDX_AHEAD];
#pragma unroll
					for (int j = 0; j < IDX_AHEAD; j++) {
						v[j] = V{};
						s[j] = 0;
						if (mk) {
							s[j] = base + 64 * k + __ffsll(mk) - 1; // < g_rows: only such lanes set a bit
							mk &= mk - 1;
							n = j + 1;
							if (live) v[j] = *(const V*)(g + (size_t)s[j] * cols + col);
						}
					}
#pragma unroll
					for (int j = 0; j < IDX_AHEAD; j++) {
						if (j < n && live) {
							const unsigned r = (unsigned)idx[s[j]] - row0; // < IDX_TILE_ROWS: the ballot's condition
#pragma unroll
							for (int e = 0; e < VEC; e++) acc[r][e][lane] += (float)v[j][e];
						}
					}
				}
			}
		}
		if (live) {
#pragma unroll
			for (int r = 0; r < IDX_TILE_ROWS; r++) {
				if (row0 + r >= (unsigned)h_rows) break;
				V o;
#pragma unroll
				for (int e = 0; e < VEC; e++) o[e] = idx_widen<T>::round(acc[r][e][lane]);
				*(V*)(h + (size_t)(row0 + r) * cols + col) = o;
			}
		}
	}
}

// ---- pad ---------------------------------------------------------------------------------------------------------------------------------------------------
enum { PAD_ZERO = 0, PAD_REPLICATE = 1 }; // CCV_NNC_PAD_* (ccv_nnc.h:98-99)
struct pad_args_t { int bd[4]; int ad[4]; int begin[4]; long sa[4], sb[4]; }; // a = the unpadded tensor, b = the padded one; extents and strides in elements of T
typedef unsigned pad_vec16_t __attribute__((ext_vector_type(4))); // eight halves moved as one element

template <typename T, int TYPE>
__global__ void __launch_bounds__(256) pad_forw_kernel(const T* a, T* b, const pad_args_t m, const size_t n)
{
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
		size_t r = idx;
		int i[4];
		i[3] = (int)(r % m.bd[3]); r /= m.bd[3];
		i[2] = (int)(r % m.bd[2]); r /= m.bd[2];
		i[1] = (int)(r % m.bd[1]); r /= m.bd[1];
		i[0] = (int)r;
		long ao = 0, bo = 0;
		bool inside = true;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			int j = i[k] - m.begin[k];
			if (TYPE == PAD_REPLICATE) j = j < 0 ? 0 : (j > m.ad[k] - 1 ? m.ad[k] - 1 : j);
			else inside = inside & (j >= 0) & (j < m.ad[k]);
			ao += (long)j * m.sa[k];
			bo += (long)i[k] * m.sb[k];
		}
		b[bo] = (TYPE == PAD_REPLICATE || inside) ? a[inside ? ao : 0] : T{};
	}
}
// h[i] = g[i + begin]
template <typename T>
__global__ void __launch_bounds__(256) pad_back_kernel(const T* g, T* h, const pad_args_t m, const size_t n)
{
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
		size_t r = idx;
		int i[4];
		i[3] = (int)(r % m.ad[3]); r /= m.ad[3];
		i[2] = (int)(r % m.ad[2]); r /= m.ad[2];
		i[1] = (int)(r % m.ad[1]); r /= m.ad[1];
		i[0] = (int)r;
		long go = 0, ho = 0;
#pragma unroll
		for (int k = 0; k < 4; k++) { go += (long)(i[k] + m.begin[k]) * m.sb[k]; ho += (long)i[k] * m.sa[k]; }
		h[ho] = g[go];
	}
}

// ---- the plans -----------------------------------------------------------------------------------------------------------------------------------------------
constexpr double IDX_MAX_ELEMENTS = 2147483648.0; // tensors of 2^31 elements and more keep their route
static inline bool idx_dense(const ccv_nnc_tensor_t* t, const int datatype) { return t && !CCV_IS_TENSOR_VIEW(t) && CCV_GET_DATA_TYPE(t->info.datatype) == datatype && t->data.u8; }
// index_select_cpu_ref.c:22-27: dim[0] rows, dim[1] columns (1-d: one column); dense tensors only, so the row stride is `cols`
static inline bool idx_rows_cols(const ccv_nnc_tensor_t* t, int* rows, int* cols)
{
	const int nd = tensor_nd(t->info.dim);
	if (nd > 2) return false;
	*rows = t->info.dim[0];
	*cols = nd < 2 ? 1 : t->info.dim[1];
	return (double)*rows * (double)*cols < IDX_MAX_ELEMENTS;
}
// table = a / h (the tensor indices point into), sel = b / g (one row per index)
struct index_plan_t { int table_rows, sel_rows, cols; const void* table; const void* sel; const void* idx; int idx_f32; };
static inline bool index_plan_fill(const ccv_nnc_tensor_t* table, const ccv_nnc_tensor_t* sel, const ccv_nnc_tensor_t* ind, index_plan_t* const o)
{
	int tc, sc;
	if (!idx_rows_cols(table, &o->table_rows, &tc) || !idx_rows_cols(sel, &o->sel_rows, &sc) || tc != sc) return false;
	if (!ind || !tensor_contiguous(ind) || tensor_count(ind->info) != (size_t)o->sel_rows) return false;
	const int it = CCV_GET_DATA_TYPE(ind->info.datatype);
	if (it != CCV_32S && it != CCV_32F) return false;
	o->cols = tc; o->table = table->data.u8; o->sel = sel->data.u8; o->idx = ind->data.u8; o->idx_f32 = it == CCV_32F;
	return table->data.u8 != sel->data.u8;
}
// true: the key is on, nothing is accumulated, table and selection are dense CCV_16F tensors (no views: the row stride is `cols`) of matching shapes with fewer
// than 2^31 elements -- *o then holds the geometry.  Backward: int32 indices only, and INDEX_BACK_TILES on (at 0 a half command keeps its fp32 images).
// false: the command keeps its present route and return value.
static bool index_half_plan(const bool forward, const int flags, const ccv_nnc_tensor_t* table, const ccv_nnc_tensor_t* sel, const ccv_nnc_tensor_t* ind, index_plan_t* const o)
{
	if (!tune(TUNE_INDEX_PAD_HALF_NATIVE) || (flags & CCV_NNC_ACCUMULATE_OUTPUT)) return false;
	if (!forward && !tune(TUNE_INDEX_BACK_TILES)) return false;
	if (!idx_dense(table, CCV_16F) || !idx_dense(sel, CCV_16F) || !index_plan_fill(table, sel, ind, o)) return false;
	return forward || !o->idx_f32;
}
// the fp32 INDEX_SELECT_BACKWARD on the tile kernel: the same refusals on CCV_32F tensors
static bool index_back_plan(const int flags, const ccv_nnc_tensor_t* h, const ccv_nnc_tensor_t* g, const ccv_nnc_tensor_t* ind, index_plan_t* const o)
{
	if (!tune(TUNE_INDEX_BACK_TILES) || (flags & CCV_NNC_ACCUMULATE_OUTPUT)) return false;
	if (!idx_dense(h, CCV_32F) || !idx_dense(g, CCV_32F) || !index_plan_fill(h, g, ind, o)) return false;
	return !o->idx_f32;
}
// elements per lane of the instance a plan runs on: 16 bytes (eight halves, four floats) where cols is a multiple and both bases are 16-byte aligned, else 1
static inline int index_vector_width(const index_plan_t& p, const int elem_size)
{
	const int w = 16 / elem_size;
	return p.cols % w == 0 && aligned16(p.table) && aligned16(p.sel) ? w : 1;
}

struct idx_prof_name_t {
	char s[96];
	idx_prof_name_t(const char* row, const char* kernel, const char* type, const int W, const char* extra) { snprintf(s, sizeof(s), "%s|nnc::%s<%s,%d%s%s>", row, kernel, type, W, extra ? "," : "", extra ? extra : ""); }
};

static int index_gather_run(const index_plan_t& p, ccv_nnc_stream_context_t* ctx)
{
	if (p.sel_rows == 0 || p.cols == 0) return CCV_NNC_EXEC_SUCCESS;
	const int W = index_vector_width(p, sizeof(half_t));
	hipStream_t stream = stream_of(ctx);
	const double moved = (double)p.sel_rows * p.cols;
	const idx_prof_name_t name("index_select_forw", "index_gather_kernel", "half", W, p.idx_f32 ? "f32" : "i32");
	note_kernel("index_gather");
	ProfScope prof(name.s, moved, sizeof(half_t) * moved * (p.idx_f32 ? 3 : 2), p.sel_rows, p.cols, p.table_rows, 1, 1, stream);
	const dim3 grid(grid_for((size_t)p.sel_rows * 64, IDX_GATHER_THREADS)), block(IDX_GATHER_THREADS);
	const half_t* const a = (const half_t*)p.table;
	half_t* const b = (half_t*)p.sel;
	if (p.idx_f32) {
		if (W == 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(index_gather_kernel<half_t, 8, float>), grid, block, 0, stream, a, (const float*)p.idx, b, p.sel_rows, p.cols, p.table_rows);
		else hipLaunchKernelGGL(HIP_KERNEL_NAME(index_gather_kernel<half_t, 1, float>), grid, block, 0, stream, a, (const float*)p.idx, b, p.sel_rows, p.cols, p.table_rows);
	} else {
		if (W == 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(index_gather_kernel<half_t, 8, int>), grid, block, 0, stream, a, (const int*)p.idx, b, p.sel_rows, p.cols, p.table_rows);
		else hipLaunchKernelGGL(HIP_KERNEL_NAME(index_gather_kernel<half_t, 1, int>), grid, block, 0, stream, a, (const int*)p.idx, b, p.sel_rows, p.cols, p.table_rows);
	}
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

template <typename T, int VEC>
static void index_scatter_launch(const index_plan_t& p, hipStream_t stream)
{
	const unsigned col_chunks = (unsigned)((p.cols + IDX_THREADS * VEC - 1) / (IDX_THREADS * VEC));
	const unsigned row_tiles = (unsigned)((p.table_rows + IDX_TILE_ROWS - 1) / IDX_TILE_ROWS);
	// tiles <= rows * cols < 2^31; the grid is capped as grid_for() caps it and the kernel strides over the tiles
	const unsigned tiles = row_tiles * col_chunks;
	const dim3 grid(grid_for((size_t)tiles * IDX_THREADS, IDX_THREADS));
	hipLaunchKernelGGL(HIP_KERNEL_NAME(index_scatter_tile_kernel<T, VEC>), grid, dim3(IDX_THREADS), 0, stream, (const T*)p.sel, (const int*)p.idx, (T*)p.table, p.sel_rows, p.table_rows, p.cols, col_chunks, tiles);
}
// h = 0, then h[idx[i]][:] += g[i][:] in row order, in one launch
template <typename T>
static int index_scatter_run(const index_plan_t& p, ccv_nnc_stream_context_t* ctx)
{
	if (p.table_rows == 0 || p.cols == 0) return CCV_NNC_EXEC_SUCCESS;
	const int W = index_vector_width(p, sizeof(T));
	hipStream_t stream = stream_of(ctx);
	const double ng = (double)p.sel_rows * p.cols, nh = (double)p.table_rows * p.cols;
	const idx_prof_name_t name("index_select_back", "index_scatter_tile_kernel", sizeof(T) == 2 ? "half" : "float", W, 0);
	note_kernel("index_scatter_tile");
	ProfScope prof(name.s, ng, sizeof(T) * (ng + nh), p.sel_rows, p.cols, p.table_rows, 1, 1, stream);
	if (W > 1) index_scatter_launch<T, 16 / sizeof(T)>(p, stream);
	else index_scatter_launch<T, 1>(p, stream);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

// ---- the pad plan --------------------------------------------------------------------------------------------------------------------------------------------
// small = the unpadded tensor (a / h), big = the padded one (b / g); strides of dense tensors or of views, in elements
static inline bool pad_args_fill(const ccv_nnc_cmd_t& cmd, const ccv_nnc_tensor_t* small, const ccv_nnc_tensor_t* big, pad_args_t* m)
{
	const int nd = tensor_nd(small->info.dim), offset = 4 - nd;
	if (nd > 4 || tensor_nd(big->info.dim) > 4) return false;
	int ss[CCV_NNC_MAX_DIM_ALLOC], sb[CCV_NNC_MAX_DIM_ALLOC];
	tensor_strides(small, ss);
	tensor_strides(big, sb);
	const int bnd = tensor_nd(big->info.dim);
	for (int k = 0; k < 4; k++) {
		const int x = k - offset, y = k - (4 - bnd);
		m->begin[k] = x >= 0 ? cmd.info.size.dim[x] : 0;
		const int end = x >= 0 ? cmd.info.pad.end[x] : 0;
		m->ad[k] = x >= 0 ? small->info.dim[x] : 1; m->sa[k] = x >= 0 ? ss[x] : 0;
		m->bd[k] = y >= 0 ? big->info.dim[y] : 1; m->sb[k] = y >= 0 ? sb[y] : 0;
		if (m->begin[k] < 0 || end < 0 || m->bd[k] != m->ad[k] + m->begin[k] + end) return false;
	}
	return true;
}
struct pad_plan_t { pad_args_t m; int type; int W; const half_t* small; const half_t* big; };
// true: the key is on, nothing is accumulated, both tensors are dense CCV_16F tensors of at most four axes and fewer than 2^31 elements, the type is zero or
// replicate -- *o then holds the arguments, in 16-byte elements (W = 8) where the innermost extents of both tensors and begin[3] are multiples of 8 and both
// bases are 16-byte aligned (replicate: and nothing is padded on the innermost axis, for a replicated edge is one element, not eight), else in halves (W = 1).
static bool pad_half_plan(const ccv_nnc_cmd_t cmd, const int flags, const ccv_nnc_tensor_t* small, const ccv_nnc_tensor_t* big, const bool forward, pad_plan_t* const o)
{
	if (!tune(TUNE_INDEX_PAD_HALF_NATIVE) || (flags & CCV_NNC_ACCUMULATE_OUTPUT)) return false;
	if (!idx_dense(small, CCV_16F) || !idx_dense(big, CCV_16F) || small->data.u8 == big->data.u8) return false;
	if (!pad_args_fill(cmd, small, big, &o->m)) return false;
	o->type = cmd.info.pad.type;
	if (forward && o->type != PAD_ZERO && o->type != PAD_REPLICATE) return false;
	pad_args_t& m = o->m;
	if ((double)m.bd[0] * m.bd[1] * m.bd[2] * m.bd[3] >= IDX_MAX_ELEMENTS) return false;
	o->small = (const half_t*)small->data.u8;
	o->big = (const half_t*)big->data.u8;
	bool vec = m.ad[3] % 8 == 0 && m.bd[3] % 8 == 0 && m.begin[3] % 8 == 0 && aligned16(o->small) && aligned16(o->big);
	if (forward && o->type == PAD_REPLICATE && m.ad[3] != m.bd[3]) vec = false;
	o->W = vec ? 8 : 1;
	if (vec) { // dense tensors: every outer stride is a multiple of the innermost extent
		m.ad[3] /= 8; m.bd[3] /= 8; m.begin[3] /= 8;
		for (int k = 0; k < 3; k++) { m.sa[k] /= 8; m.sb[k] /= 8; }
	}
	return true;
}
template <typename T>
static void pad_launch(const pad_args_t& m, const int type, const bool forward, const void* small, const void* big, const size_t n, hipStream_t stream)
{
	const dim3 grid(grid_for(n, 256)), block(256);
	if (!forward) hipLaunchKernelGGL(HIP_KERNEL_NAME(pad_back_kernel<T>), grid, block, 0, stream, (const T*)big, (T*)small, m, n);
	else if (type == PAD_ZERO) hipLaunchKernelGGL(HIP_KERNEL_NAME(pad_forw_kernel<T, PAD_ZERO>), grid, block, 0, stream, (const T*)small, (T*)big, m, n);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(pad_forw_kernel<T, PAD_REPLICATE>), grid, block, 0, stream, (const T*)small, (T*)big, m, n);
}
static int pad_half_run(const pad_plan_t& p, const bool forward, ccv_nnc_stream_context_t* ctx)
{
	const pad_args_t& m = p.m;
	const size_t n = forward ? (size_t)m.bd[0] * m.bd[1] * m.bd[2] * m.bd[3] : (size_t)m.ad[0] * m.ad[1] * m.ad[2] * m.ad[3]; // elements of T written
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	hipStream_t stream = stream_of(ctx);
	const double na = (double)m.ad[0] * m.ad[1] * m.ad[2] * m.ad[3] * p.W, nb = (double)m.bd[0] * m.bd[1] * m.bd[2] * m.bd[3] * p.W;
	const idx_prof_name_t name(forward ? "pad_forw" : "pad_back", forward ? "pad_forw_kernel" : "pad_back_kernel", "half", p.W, !forward ? 0 : (p.type == PAD_ZERO ? "zero" : "replicate"));
	note_kernel(forward ? "pad_forw_half" : "pad_back_half");
	ProfScope prof(name.s, forward ? nb : na, sizeof(half_t) * (forward ? na + nb : 2 * na), m.bd[0], m.bd[1], m.bd[2], m.bd[3] * p.W, 1, stream);
	if (p.W == 8) pad_launch<pad_vec16_t>(m, p.type, forward, p.small, p.big, n, stream);
	else pad_launch<half_t>(m, p.type, forward, p.small, p.big, n, stream);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

} // namespace nnc
