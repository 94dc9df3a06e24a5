// b[M, N] = a[M, K] . w[N, K]^T (+ bias[N]) for a dense layer (ccv_cnnp_dense) whose weight is a DENSE CCV_16F matrix and whose activations are a few CCV_16F rows
// (1 <= M <= 32: token-by-token decoding, small batches).  The problem is a stream: 2 N K bytes of weight read once, a few KB of activations, negligible arithmetic.
// The general contraction core (gemm_launch.h: a 64 x 64 tile, both operands through LDS, split-K slabs and splitk_reduce_kernel) pads at least half its tile at
// these shapes.  cmd_gemm.cpp decides which commands come here (gemm_rows_fused; tunables GEMM_F16_ROWS, GEMM_F16_ROWS_SLICES).  Sums are fp32 on
// v_mfma_f32_32x32x16_f16 (isa.h nnc_mfma_f16), each result is rounded to half once.
//
// Weight: memory -> registers -> matrix instruction, no LDS in its path.  Operand B of the instruction is 32 consecutive weight rows (column n = n0 + (lane & 31)),
// lanes 0 .. 31 supply eight consecutive k, lanes 32 .. 63 the next eight: ONE 16-byte load of a weight row (a "group" of eight k) is one lane's operand of one
// step; the two halves of a wave read neighbouring groups, a wave's load instruction reads 32 bytes of each of the tile's 32 rows.  w may be a view: its row
// stride any multiple of 8 (rows stay 16-byte aligned); only groups k < K of rows n < N are ever read, so nothing past the last byte of w.
//
// Work split.  A workgroup of four waves owns a tile of 32 weight rows over one slice of K and walks the slice in chunks of 64 groups (512 k); within a chunk wave v
// owns the 8 steps 8 v .. 8 v + 7, that is 256 consecutive bytes of each row (two cache lines, each fetched by one wave).  The four accumulators meet in LDS in
// wave order.  The grid is (tiles of N) x (slices of K).  With one slice the workgroup adds the bias and writes halves; otherwise the slices write fp32 partials
// [slice][M][N] into the stream's workspace and gemm_rows_fold_kernel adds them in slice order, adds the bias and rounds once.  No atomics: every sum has one
// order, fixed by the shapes and the slice count -- two runs give the same bits.
//
// Loads in flight.  A lane holds 2 x 8 weight registers of 16 bytes (64 VGPRs): the slots of chunks c and c + 1.  The step that consumes a slot of chunk c refills
// it with the same step of chunk c + 2, so the loads of the next chunk (and, as issued, of the one after) are in flight during a chunk's matrix steps.  Every load
// is unconditional (clamped addresses, below) so that the compiler can wait BY COUNT; what it emits for gfx950 (s_waitcnt vmcnt in the assembly, hipcc -O3):
//   * in front of the matrix steps the waits are counted (AP = 1: vmcnt 8, 7, 7, 6 .. 2 down the 8 steps of one chunk, none in the other; AP = 8: vmcnt 8 once);
//   * the store of the staged activations waits for their loads, which were issued at the top of the chunk: everything OLDER -- the other ring half, which the
//     next chunk is about to use -- has then landed too, and only this chunk's refills stay in flight across the store and the barrier: 8 of them for AP = 8
//     (vmcnt 15 .. 8 in front of the 8 stores), but 2 for AP = 1, where the compiler moves six of the eight refills behind the store;
//   * so a lane has 8 to 16 (+ AP) sixteen-byte loads in flight during the steps and 2 (AP = 1) to 8 (AP = 8) at the store, once per chunk: a refill has one
//     chunk's time to land, not two.  The ring's second half buys the overlap of the steps with the next chunk's loads, not a second chunk of latency.
// The price, as the build prints it (NumVgprs + NumAgprs = total, Occupancy in waves a SIMD; no scratch; the accumulator lives in AGPRs, once per ring half):
//   AP = 1: 107 + 32 = 139, 3    AP = 2: 130 + 32 = 162, 3    AP = 4: 144 + 32 = 176, 2    AP = 8: 170 + 32 = 202, 2
// gemm_qx_f16.h, which this kernel follows in its tile and its fold, holds 8 loads a lane and waits for all of them (vmcnt 0) once per chunk.
//
// Activations: once per workgroup and chunk.  The chunk's a[0 .. 4 AP) x 512 k goes memory -> registers -> LDS (thread t stages the 16-byte pieces t, t + 256, ...:
// piece i = row i / 64, group i % 64), double-buffered: the loads of chunk c + 1 are issued in front of chunk c's matrix steps and stored behind them, one
// LDS-only barrier per chunk (NNC_LDS_BARRIER: the weight loads stay in flight across it).  AP = 1, 2, 4, 8 (template) for M <= 4, 8, 16, 32: 8.1 / 16.3 / 32.5 /
// 65 KB of LDS (at least the 12 KB the accumulators meet in).  Rows are GR_PITCH = 520 halves apart (16 bytes of padding: the 32 lanes of a 16-byte LDS read land
// in different banks).  A lane of a group past the slice's end supplies zeros in both operands; rows r >= M are never read from a (clamped addresses, below).
#pragma once
#include "common.h"
#include "isa.h"

namespace nnc {

constexpr int GR_THREADS = 256, GR_WAVES = GR_THREADS / 64;
constexpr int GR_TILE_N = 32; // weight rows of a workgroup: the matrix instruction's column count
constexpr int GR_MAX_M = 32;  // activation rows: its row count
constexpr int GR_UNROLL = 8;  // steps of a wave per chunk
constexpr int GR_CHUNK_GROUPS = 2 * GR_WAVES * GR_UNROLL; // groups of eight k per chunk (64: 512 k)
constexpr int GR_PITCH = 8 * GR_CHUNK_GROUPS + 8; // halves from one staged row of a to the next
// The launch's slice rule (gemm_rows_f16_run): workgroups for GR_WG_PER_CU a CU, no slice shorter than a chunk, the partials' traffic (8 M N bytes a slice, written
// and read) at most an eighth of the weight's 2 N K bytes, never more than GR_MAX_SLICES (the fold holds a row of them in registers, eight loads at a time)
constexpr int GR_WG_PER_CU = 1; // (measured, DESIGN.md section 5: long slices keep the loads flowing; two a CU was 8 % slower at N = K = 4096)
constexpr int GR_MAX_SLICES = 32;

struct gr_geom_t {
	const half_t* w; long ldw; // [N][K], rows ldw halves apart (a multiple of 8, base 16-byte aligned)
	const half_t* a; long lda; // [M][K], the same
	const half_t* bias;        // null, or N halves
	half_t* b; long ldb;
	float* partial;            // null (one slice: the kernel writes b), or [slices][M][N]
	int M, N, KG;              // KG = K / 8 groups per row
	int slice_groups;          // groups per slice (even; the last slice may be shorter)
};

__device__ __forceinline__ halfx8 gr_zero8()
{
	halfx8 z;
#pragma unroll
	for (int e = 0; e < 8; e++) z[e] = (half_t)0.f;
	return z;
}
// v, or zeros: the loads themselves are never conditional (a branch around a load makes the compiler wait for EVERY load in flight, vmcnt(0), at the next use)
__device__ __forceinline__ halfx8 gr_keep8(const halfx8 v, const bool ok) { return ok ? v : gr_zero8(); }

// Every load below is unconditional and in bounds by a CLAMPED address: a group past the slice's end reads the slice's last group again, a row past the last the
// last row -- only groups k < K of rows n < N of w and rows m < M of a are ever read.  What a clamped lane holds is then replaced by zeros in BOTH operands where
// the group is past the slice (0 x inf), and left alone where only the row is (a row m >= M or a column n >= N of the product is never stored).
// The staging registers <- the chunk at group C0 of a: piece i = tid + 256 p is row i / 64, group C0 + i % 64
#define GR_FETCH_A(C0) do { \
		_Pragma("unroll") for (int p = 0; p < AP; p++) { \
			const int i = tid + GR_THREADS * p, r = i >> 6, gi = (C0) + (i & 63); \
			ar[p] = *(const halfx8*)(g.a + (long)(r < g.M ? r : g.M - 1) * g.lda + 8 * (long)(gi < g_hi ? gi : g_hi - 1)); \
		} \
	} while (0)
#define GR_STORE_A(BUF) do { \
		_Pragma("unroll") for (int p = 0; p < AP; p++) { \
			const int i = tid + GR_THREADS * p; \
			*(halfx8*)(abuf + (BUF) * A_BUF + (i >> 6) * GR_PITCH + 8 * (i & 63)) = ar[p]; \
		} \
	} while (0)
// Slot u of ring half SET <- the lane's group of step u of the chunk at C0
#define GR_FETCH_W(SET, u, C0) do { \
		const int gi = (C0) + my_group + 2 * (u); \
		wr[SET][u] = *(const halfx8*)(w_row + 8 * (long)(gi < g_hi ? gi : g_hi - 1)); \
	} while (0)
// One chunk: the next chunk's activations requested, then the wave's 8 steps, each refilling its slot with the chunk after the next, then the activations stored
#define GR_CHUNK(SET, C0) do { \
		GR_FETCH_A((C0) + GR_CHUNK_GROUPS); \
		_Pragma("unroll") for (int u = 0; u < GR_UNROLL; u++) { \
			const bool ok = (C0) + my_group + 2 * u < g_hi; \
			const halfx8 av = gr_keep8(*(const halfx8*)(a_lane + (SET) * A_BUF + 16 * u), ok); \
			acc = nnc_mfma_f16(av, gr_keep8(wr[SET][u], ok), acc); \
			GR_FETCH_W(SET, u, (C0) + 2 * GR_CHUNK_GROUPS); \
		} \
		GR_STORE_A((SET) ^ 1); \
		NNC_LDS_BARRIER(); \
	} while (0)

template <int AP>
__global__ void __launch_bounds__(GR_THREADS) gemm_rows_f16_kernel(const gr_geom_t g)
{
	constexpr int A_BUF = 4 * AP * GR_PITCH; // halves of one buffer of a: 4 AP rows
	constexpr int A_BYTES = 2 * A_BUF * (int)sizeof(half_t), RED_BYTES = (GR_WAVES - 1) * 16 * 64 * (int)sizeof(float);
	__shared__ __attribute__((aligned(16))) unsigned char lds[A_BYTES > RED_BYTES ? A_BYTES : RED_BYTES];
	half_t* const abuf = (half_t*)lds; // [2][4 AP][GR_PITCH]
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int j = lane & 31, hi = lane >> 5;
	const int n0 = blockIdx.x * GR_TILE_N, n = n0 + j;
	const int g_lo = blockIdx.y * g.slice_groups;
	const int g_hi = g_lo + g.slice_groups < g.KG ? g_lo + g.slice_groups : g.KG;
	const bool row_ok = n < g.N, a_ok = j < g.M; // (M <= 4 AP: a lane with a_ok has a staged row)
	const int my_group = 2 * GR_UNROLL * wave + hi; // the lane's group of step 0 within a chunk; step u: + 2 u
	const half_t* const w_row = g.w + (long)(row_ok ? n : g.N - 1) * g.ldw;
	const half_t* const a_lane = abuf + (a_ok ? j : 0) * GR_PITCH + 8 * my_group; // (a lane without a row reads row 0: its products are never stored)
	halfx8 wr[2][GR_UNROLL], ar[AP];
	floatx16 acc;
#pragma unroll
	for (int r = 0; r < 16; r++) acc[r] = 0.f;
	// prologue: the ring filled with the slice's first two chunks, its first chunk of a staged
#pragma unroll
	for (int u = 0; u < GR_UNROLL; u++) GR_FETCH_W(0, u, g_lo);
	GR_FETCH_A(g_lo);
#pragma unroll
	for (int u = 0; u < GR_UNROLL; u++) GR_FETCH_W(1, u, g_lo + GR_CHUNK_GROUPS);
	GR_STORE_A(0);
	NNC_LDS_BARRIER();
	for (int c0 = g_lo; c0 < g_hi; c0 += 2 * GR_CHUNK_GROUPS) { // (two chunks a trip: the ring's halves are named, never indexed)
		GR_CHUNK(0, c0);
		if (c0 + GR_CHUNK_GROUPS >= g_hi) break; // (the same for the whole workgroup)
		GR_CHUNK(1, c0 + GR_CHUNK_GROUPS);
	}
	// (every chunk ended with a barrier behind its LDS reads: the accumulators of waves 1 .. 3 take the activations' place)
	float* const red = (float*)lds; // [GR_WAVES - 1][16][64]
	if (wave > 0)
#pragma unroll
		for (int r = 0; r < 16; r++) red[((wave - 1) * 16 + r) * 64 + lane] = acc[r];
	__syncthreads();
	if (wave > 0 || !row_ok) return;
#pragma unroll
	for (int v = 0; v < GR_WAVES - 1; v++)
#pragma unroll
		for (int r = 0; r < 16; r++) acc[r] += red[(v * 16 + r) * 64 + lane];
	const float bias = g.bias && !g.partial ? (float)g.bias[n] : 0.f;
#pragma unroll
	for (int r = 0; r < 16; r++) {
		const int m = (r & 3) + 8 * (r >> 2) + 4 * hi; // the accumulator's row (isa.h)
		if (m >= g.M) continue;
		if (g.partial) g.partial[((size_t)blockIdx.y * (size_t)g.M + (size_t)m) * (size_t)g.N + (size_t)n] = acc[r];
		else g.b[(long)m * g.ldb + n] = (half_t)(acc[r] + bias);
	}
}
#undef GR_CHUNK
#undef GR_FETCH_W
#undef GR_STORE_A
#undef GR_FETCH_A

// b[m][n] = half(partial[0][m][n] + partial[1][m][n] + ... (in slice order) + bias[n]).  A thread owns one element and requests eight slices' values before it adds
// the first: the adds keep slice order, the trips to memory do not form a chain (sdpa_decode_f16.h's fold walks its splits one trip after the other: 0.5 us a split).
__global__ void __launch_bounds__(256) gemm_rows_fold_kernel(const float* const partial, const int slices, const int M, const int N, const half_t* const bias, half_t* const b, const long ldb)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= M * N) return;
	const int m = i / N, n = i - m * N;
	const size_t plane = (size_t)M * (size_t)N;
	float s = partial[i];
	for (int k0 = 1; k0 < slices; k0 += 8) {
		float v[8];
#pragma unroll
		for (int k = 0; k < 8; k++) v[k] = k0 + k < slices ? partial[(size_t)(k0 + k) * plane + (size_t)i] : 0.f;
#pragma unroll
		for (int k = 0; k < 8; k++) if (k0 + k < slices) s += v[k];
	}
	if (bias) s += (float)bias[n];
	b[(long)m * ldb + n] = (half_t)s;
}

template <int AP>
static void gemm_rows_launch(const gr_geom_t& g, const int tiles, const int slices, hipStream_t stream)
{
	hipLaunchKernelGGL(HIP_KERNEL_NAME(gemm_rows_f16_kernel<AP>), dim3((unsigned)tiles, (unsigned)slices), dim3(GR_THREADS), 0, stream, g);
}

// The launch.  The caller has checked the operands (cmd_gemm.cpp gemm_rows_fused); here the slices.
static int gemm_rows_f16_run(const half_t* const w, const long ldw, const half_t* const a, const long lda, const half_t* const bias, half_t* const b, const long ldb, const int M, const int N, const int K, ccv_nnc_stream_context_t* const ctx)
{
	gr_geom_t g;
	g.w = w; g.ldw = ldw; g.a = a; g.lda = lda; g.bias = bias; g.b = b; g.ldb = ldb; g.partial = 0;
	g.M = M; g.N = N; g.KG = K / 8;
	const int tiles = (N + GR_TILE_N - 1) / GR_TILE_N;
	long slices = tune(TUNE_GEMM_F16_ROWS_SLICES);
	if (slices <= 0) { // the rule written down at GR_WG_PER_CU
		slices = ((long)GR_WG_PER_CU * device_cu_count() + tiles - 1) / tiles;
		if (slices > g.KG / GR_CHUNK_GROUPS) slices = g.KG / GR_CHUNK_GROUPS;
		if (slices > K / (32l * M)) slices = K / (32l * M);
	}
	if (slices > GR_MAX_SLICES) slices = GR_MAX_SLICES;
	if (slices > g.KG) slices = g.KG;
	if (slices < 1) slices = 1;
	g.slice_groups = (int)(((g.KG + slices - 1) / slices + 1) & ~1l);
	slices = (g.KG + g.slice_groups - 1) / g.slice_groups;
	hipStream_t stream = stream_of(ctx);
	if (slices > 1) {
		g.partial = (float*)workspace_of(ctx, sizeof(float) * (size_t)slices * (size_t)M * (size_t)N);
		if (!g.partial) return CCV_NNC_EXEC_OOM;
	}
	note_kernel("gemm_rows_f16");
	const int ap = M <= 4 ? 1 : (M <= 8 ? 2 : (M <= 16 ? 4 : 8));
	char prof_name[192];
	snprintf(prof_name, sizeof(prof_name), "gemm_fwd|nnc::gemm_rows_f16_kernel<%d> EPI = %s", ap, slices <= 1 ? "EpiStoreH" : "EpiPartialH");
	{
		ProfScope prof(prof_name, 2.0 * (double)M * (double)N * (double)K, 2.0 * ((double)N * K + (double)M * K + (double)M * N), M, N, K, 1, (int)slices, stream);
		switch (ap) {
			case 1: gemm_rows_launch<1>(g, tiles, (int)slices, stream); break;
			case 2: gemm_rows_launch<2>(g, tiles, (int)slices, stream); break;
			case 4: gemm_rows_launch<4>(g, tiles, (int)slices, stream); break;
			default: gemm_rows_launch<8>(g, tiles, (int)slices, stream); break;
		}
	}
	HIP_ENFORCE(hipGetLastError());
	if (slices > 1) {
		hipLaunchKernelGGL(gemm_rows_fold_kernel, dim3((unsigned)(((long)M * N + 255) / 256)), dim3(256), 0, stream, (const float*)g.partial, (int)slices, M, N, bias, b, ldb);
		HIP_ENFORCE(hipGetLastError());
	}
	return CCV_NNC_EXEC_SUCCESS;
}

} // namespace nnc
