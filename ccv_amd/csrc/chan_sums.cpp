// The slice plan of the column sums, what they take from the workspace, and the five sums the commands call (chan_sums.h says what lives where).
#include "chan_sums.h"

namespace nnc {

// the slices a plan starts from: with the column tiles, about four workgroups per CU
static long colsum_slices_most(const long col_tiles) { return col_tiles > 0 ? ((long)device_cu_count() * 4 + col_tiles - 1) / col_tiles : 1; }
colsum_plan_t colsum_plan(const long rows, const int cols)
{
	colsum_plan_t p;
	p.col_tiles = (cols + RC_COLS - 1) / RC_COLS;
	long slices = colsum_slices_most(p.col_tiles);
	const long max_slices = (rows + 63) / 64;
	if (slices > max_slices) slices = max_slices;
	if (slices < 1) slices = 1;
	p.rows_per_slice = (rows + slices - 1) / slices;
	if (p.rows_per_slice < 1) p.rows_per_slice = 1; // (no rows: one slice of nothing)
	p.slices = rows > 0 ? (rows + p.rows_per_slice - 1) / p.rows_per_slice : 1; // re-derived: no slice is empty
	return p;
}
size_t colsum_workspace_bytes(const long rows, const int cols) { return sizeof(float) * (size_t)colsum_plan(rows, cols).slices * (size_t)cols; }
// sizeof(float) * ceil(cu * 4 / col_tiles) * cols.  The plan starts from s0 = ceil(cu * 4 / col_tiles) slices and only ever lowers that: the cap rows / 64
// lowers it, and the slices re-derived from rows_per_slice = ceil(rows / s) number ceil(rows / rows_per_slice) <= s.  So s0 bounds every plan of `cols` columns;
// and it is reached (rows = 64 * s0 * s0 gives s0 slices of 64 * s0 rows each), so it is the maximum, not an estimate.
size_t colsum_workspace_bound(const int cols) { return cols > 0 ? sizeof(float) * (size_t)colsum_slices_most((cols + RC_COLS - 1) / RC_COLS) * (size_t)cols : 0; }

// Slices per plane: none for planes of at most CHAN_RUN_SLICE elements or when the planes alone give CHAN_SLICE_WAVES_PER_CU waves per CU; else as many as
// that takes, at most ceil(inner / CHAN_RUN_SLICE) of them, each a multiple of eight elements, none empty.
plane_slices_t chan_plane_slices(const long planes, const long inner)
{
	plane_slices_t r = { 1, inner };
	if (inner <= CHAN_RUN_SLICE || planes < 1) return r;
	const long want = ((long)device_cu_count() * CHAN_SLICE_WAVES_PER_CU + planes - 1) / planes, most = (inner + CHAN_RUN_SLICE - 1) / CHAN_RUN_SLICE;
	long slices = want < most ? want : most;
	if (slices <= 1) return r;
	r.per = ((inner + slices - 1) / slices + 7) & ~7L;
	r.slices = (inner + r.per - 1) / r.per;
	return r;
}

// The per-image product sums: the tile width among 8, 16, 32, 64 channel vectors that wastes the fewest lanes on the last tile (the widest of equals; fewer than
// 8 vectors: the next power of two), then pixel slices until the launch has about four workgroups per CU, none with fewer than four pixels per phase.
scaled_rows_plan_t scaled_rows_plan(const int N, const int cv, const long P)
{
	scaled_rows_plan_t sp;
	sp.cvt_log2 = 0;
	if (cv < 8) { while ((1 << sp.cvt_log2) < cv) sp.cvt_log2++; }
	else {
		long best = -1;
		for (int l = 3; l <= 6; l++) {
			const long w = 1L << l, covered = w * ((cv + w - 1) / w);
			if (best < 0 || covered * 1 <= best) { best = covered; sp.cvt_log2 = l; }
		}
	}
	const int cvt = 1 << sp.cvt_log2, phases = 256 / cvt;
	sp.tiles = (cv + cvt - 1) / cvt;
	const long wgs = (long)N * sp.tiles;
	long slices = wgs > 0 ? ((long)device_cu_count() * 4 + wgs - 1) / wgs : 1;
	const long max_slices = (P + 4L * phases - 1) / (4L * phases);
	if (slices > max_slices) slices = max_slices;
	if (slices < 1) slices = 1;
	sp.rows_per_slice = (P + slices - 1) / slices;
	if (sp.rows_per_slice < 1) sp.rows_per_slice = 1;
	sp.slices = P > 0 ? (P + sp.rows_per_slice - 1) / sp.rows_per_slice : 1;
	return sp;
}

// Many slices (one per image and 64-pixel tile: thousands) are first folded in groups -- a workgroup per (64 columns, group of slices), four slices in flight per
// column, coalesced rows -- so that the final kernel's per-column chains stay a few loads long.  Fixed order throughout: deterministic.
struct partials_groups_t { int group; long groups; }; // groups == 0: few enough slices for the fold alone
static partials_groups_t partials_groups(const long slices)
{
	partials_groups_t r = { 0, 0 };
	if (slices > 512) {
		r.group = (int)((slices + 255) / 256 < 16 ? 16 : (slices + 255) / 256);
		r.groups = (slices + r.group - 1) / r.group;
	}
	return r;
}
size_t colsum_partials_bytes(const long slices, const int cols) { return sizeof(float) * (size_t)(slices + partials_groups(slices).groups) * (size_t)cols; }
static __global__ void __launch_bounds__(256) partials_group_kernel(const float* __restrict__ in, const long slices, const int cols, const int group, float* __restrict__ out)
{
	__shared__ float red[4][64];
	const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
	const int c = blockIdx.x * 64 + cl;
	const long s0 = (long)blockIdx.y * group, s1 = s0 + group < slices ? s0 + group : slices;
	float a = 0.f, b = 0.f;
	if (c < cols) {
		long i = s0 + ph;
		for (; i + 4 < s1; i += 8) { a += in[i * cols + c]; b += in[(i + 4) * cols + c]; }
		if (i < s1) a += in[i * cols + c];
	}
	red[ph][cl] = a + b;
	__syncthreads();
	if (ph == 0 && c < cols) out[(long)blockIdx.y * cols + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// 16-byte variant of the rows kernel for plain float sums (cols % 4 == 0, ld % 4 == 0, 16-byte aligned): 16 lanes x float4 cover the 64 columns of a tile,
// the other 16 lane groups of the block walk 16 row phases; fixed-order fold of the phases through LDS.
static __global__ void __launch_bounds__(256) colsum_partial_v4_kernel(const float* x, const long rows, const int cols, const long ld, const long rows_per_slice, float* partial)
{
	__shared__ float4 red[16][16];
	const int q = threadIdx.x & 15, phase = threadIdx.x >> 4;
	const int c = blockIdx.x * RC_COLS + q * 4;
	const long r0 = (long)blockIdx.y * rows_per_slice;
	long r1 = r0 + rows_per_slice;
	if (r1 > rows) r1 = rows;
	float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
	if (c < cols)
		for (long r = r0 + phase; r < r1; r += 16) {
			const float4 v = *(const float4*)(x + r * ld + c);
			s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
		}
	red[phase][q] = s;
	__syncthreads();
	if (phase == 0 && c < cols) {
		float4 t = red[0][q];
		for (int p = 1; p < 16; p++) { const float4 u = red[p][q]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
		*(float4*)(partial + (long)blockIdx.y * cols + c) = t;
	}
}

int colsum_f32(const float* x, long rows, int cols, long ld, float* out, int accumulate, ccv_nnc_stream_context_t* ctx)
{
	if (cols <= 0) return CCV_NNC_EXEC_SUCCESS;
	const colsum_plan_t p = colsum_plan(rows, cols);
	float* const partial = (float*)workspace_of(ctx, colsum_workspace_bytes(rows, cols));
	if (!partial) return CCV_NNC_EXEC_OOM;
	hipStream_t stream = stream_of(ctx);
	const dim3 grid(p.col_tiles, (unsigned)p.slices);
	if (cols % 4 == 0 && ld % 4 == 0 && aligned16(x) && aligned16(partial))
		hipLaunchKernelGGL(colsum_partial_v4_kernel, grid, dim3(256), 0, stream, x, rows, cols, ld, p.rows_per_slice, partial);
	else
		hipLaunchKernelGGL(HIP_KERNEL_NAME(chan_reduce_rows_kernel<RSum, false, float>), grid, dim3(256), 0, stream, RSum(), x, (const float*)0, rows, cols, ld, p.rows_per_slice, partial);
	HIP_ENFORCE(hipGetLastError());
	return chan_fold(partial, p.slices, cols, out, accumulate, stream);
}
int colsum_f16(const void* x, long rows, int cols, long ld, void* out, int accumulate, ccv_nnc_stream_context_t* ctx)
{ // always the scalar kernel: the 16-byte one folds 16 row phases where this one folds 4
	if (cols <= 0) return CCV_NNC_EXEC_SUCCESS;
	return chan_reduce_rows<RSum, false>(RSum(), (const half_t*)x, (const half_t*)0, rows, cols, ld, (half_t*)out, accumulate, ctx);
}
int colsum_partials_f16(const float* partial, long slices, const int cols, void* out, const int accumulate, ccv_nnc_stream_context_t* ctx)
{
	if (cols <= 0) return CCV_NNC_EXEC_SUCCESS;
	if (slices > 0x7fffffffL) return CCV_NNC_EXEC_INVALID;
	hipStream_t stream = stream_of(ctx);
	const partials_groups_t pg = partials_groups(slices);
	if (pg.groups) { // (the grouped sums go to a second area right behind the partials: colsum_partials_bytes)
		float* const folded = (float*)partial + (size_t)slices * cols;
		hipLaunchKernelGGL(partials_group_kernel, dim3((cols + 63) / 64, (unsigned)pg.groups), dim3(256), 0, stream, partial, slices, cols, pg.group, folded);
		HIP_ENFORCE(hipGetLastError());
		partial = folded;
		slices = pg.groups;
	}
	return chan_fold(partial, slices, cols, (half_t*)out, accumulate, stream);
}
int chan_sum_planes(const float* x, long outer, int C, long inner, float* out, int accumulate, ccv_nnc_stream_context_t* ctx)
{
	const chan_view_t v = { outer, C, inner };
	return chan_reduce<RSum, false>(RSum(), x, (const float*)0, v, out, ctx, accumulate);
}
int chan_sum_planes_f16(const void* x, long outer, int C, long inner, void* out, int accumulate, ccv_nnc_stream_context_t* ctx)
{ // a wave per plane whatever `inner` is
	if (C <= 0 || outer <= 0) return CCV_NNC_EXEC_SUCCESS;
	const chan_view_t v = { outer, C, inner };
	return chan_reduce_planes<RSum, false>(RSum(), (const half_t*)x, (const half_t*)0, v, (half_t*)out, accumulate, ctx);
}

} // namespace nnc

// Test hook: the plan and the workspace figures for one shape (host arithmetic only, nothing is launched).
extern "C" void nnc_mi355x_debug_colsum_plan(long rows, int cols, long* slices, long* rows_per_slice, size_t* bytes, size_t* bound)
{
	const nnc::colsum_plan_t p = nnc::colsum_plan(rows, cols);
	*slices = p.slices;
	*rows_per_slice = p.rows_per_slice;
	*bytes = nnc::colsum_workspace_bytes(rows, cols);
	*bound = nnc::colsum_workspace_bound(cols);
}
