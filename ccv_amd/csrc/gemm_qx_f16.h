// b[M, N] = a[M, K] . w[N, K]^T (+ bias) for a dense layer whose weight is PALETTIZED (CCV_QX with a half palette: 4 .. 8-bit indices into per-block palettes,
// palette.cpp has the layout) and whose activations are a few CCV_16F rows (token-by-token decoding, small batches): the weight is read as its byte stream and
// decoded on the way into the matrix instruction -- q / 8 bytes of HBM traffic per weight element, where expanding it first (depalettized_exec) costs q / 8 + 2
// written + 2 read again.  cmd_gemm.cpp decides which commands come here (tunables GEMM_QX_FUSED, GEMM_QX_SLICES).
//
// Operands of v_mfma_f32_32x32x16_f16 (isa.h nnc_mfma_f16): A = the activation rows (row m = lane & 31, zero for m >= M), B = 32 decoded weight rows (column
// n = n0 + (lane & 31)); lanes 0 .. 31 supply eight consecutive k, lanes 32 .. 63 the next eight.  Eight consecutive k of one weight row are exactly ONE index group
// of the stream (K and number_in_blocks are multiples of eight: a group never straddles a row or a block), so a lane's B operand is
//   one unaligned 8-byte load of the group's Q index bytes (group_bits, palette_bits.h: byte loads of only the group's own bytes where the eight would reach
//   past the stream's end), one byte swap, a constant shift + mask per element, eight 2-byte look-ups in LDS;
// its A operand is one 16-byte load of a.  The lane ends up with b[m][n0 + (lane & 31)] for 16 values of m: consecutive lanes store consecutive halves.
//
// Work split.  A workgroup of four waves owns a tile of 32 weight rows over one slice of K and walks the slice in chunks of up to 64 groups (512 k): wave v takes
// the chunk's MFMA steps v, v + 4, ... (neighbouring waves read neighbouring bytes of each row), issues the index and activation loads of all its eight steps,
// and only then the workgroup stages the chunk's palettes in LDS (16 bytes a lane) -- one round trip to memory per chunk; two, with the palettes staged first, ran
// 1.5x - 2x slower.  The four accumulators meet in LDS in wave order.  The grid is (tiles of N) x (slices of K): N / 32 tiles alone are fewer
// than the CUs for a transformer's layers, the slices fill the device.  With one slice the workgroup adds the bias and writes halves; otherwise slices write fp32
// partials into the stream's workspace and gemm_qx_fold_kernel adds them in slice order, adds the bias and rounds once.  No atomics: every sum has one order,
// fixed by the shapes -- two runs give the same bits.
//
// Palettes in LDS (QX_LDS_BYTES = 32 KiB a workgroup: five workgroups a CU).  Which blocks a chunk needs depends on how blocks and rows interleave:
//   dense   slot = block - (the tile's first block of the chunk): every block from the first row's to the last row's.  Blocks as large as rows or larger.
//   sparse  slot = row * ppr + (block - the row's first block of the chunk), ppr = the most blocks len consecutive elements touch.  Blocks smaller than rows.
// The launch takes whichever needs fewer slots, and halves the chunk until they fit; a command whose palettes do not fit at two groups a chunk (8-bit indices in
// blocks of eight would need 64 KiB) is refused, not spilled.  A block's stride may be odd (five index bytes for eight 5-bit elements): palette words are read
// unaligned, as depalettize_kernel reads them.
#pragma once
#include "common.h"
#include "isa.h"
#include "palette_bits.h"

namespace nnc {

constexpr int QX_THREADS = 256, QX_WAVES = QX_THREADS / 64;
constexpr int QX_TILE_N = 32;        // weight rows of a workgroup: the matrix instruction's column count
constexpr int QX_MAX_M = 32;         // activation rows: its row count
constexpr int QX_LDS_BYTES = 32768;  // palettes a workgroup may stage (the accumulators of waves 1 .. 3 meet in the same bytes afterwards: 12 KiB)
constexpr int QX_UNROLL = 8;        // MFMA steps of a wave per chunk: their index and activation loads are all in flight before the first look-up
constexpr int QX_CHUNK_GROUPS = 2 * QX_WAVES * QX_UNROLL; // groups of eight k per chunk, at most (64: 512 k)
constexpr int QX_MIN_SLICE_GROUPS = 64; // the launch's own slice rule never cuts K finer than this

struct qx_geom_t {
	const unsigned char* w; // the stream
	size_t in_len;          // its bytes
	size_t block_stride;    // bytes from one block to the next: palette + a full block's index bytes
	const half_t* a; long lda;
	const half_t* bias;     // null, or N halves
	half_t* b; long ldb;
	float* partial;         // null (one slice: the kernel writes b), or [slices][M][N]
	int M, N, KG;           // KG = K / 8 groups per weight row
	int gpb;                // groups per block
	unsigned blocks;        // blocks of the stream
	unsigned div_m; int div_sh; // G / gpb for a group index G < 2^31 as (G * div_m) >> div_sh (round-up reciprocal, as palette.cpp's)
	int slice_groups;       // groups per slice (even; the last slice may be shorter)
	int chunk_groups;       // groups per chunk (even)
	int dense, ppr, npal;   // the slot rule above; npal slots are staged per chunk
	unsigned ppr_m;         // p / ppr for a slot p < 2048 as (p * ppr_m) >> 20
};
typedef unsigned qx_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned qx_block_of(const qx_geom_t& g, const unsigned G) { return (unsigned)(((unsigned long long)G * g.div_m) >> g.div_sh); }

template <int Q>
__global__ void __launch_bounds__(QX_THREADS) gemm_qx_f16_kernel(const qx_geom_t g)
{
	__shared__ __attribute__((aligned(16))) unsigned char lds[QX_LDS_BYTES];
	half_t* const pal = (half_t*)lds; // [npal][1 << Q]
	constexpr unsigned MASK = (1u << Q) - 1;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int j = lane & 31, hi = lane >> 5;
	const int n0 = blockIdx.x * QX_TILE_N, n = n0 + j;
	const int g_lo = blockIdx.y * g.slice_groups;
	const int g_hi = g_lo + g.slice_groups < g.KG ? g_lo + g.slice_groups : g.KG;
	const bool row_ok = n < g.N, a_ok = j < g.M;
	const unsigned row_g0 = (unsigned)n * (unsigned)g.KG; // the row's first group in the stream's group numbering
	const half_t* const a_row = g.a + (long)j * g.lda;
	const int slot_base = g.dense ? 0 : j * g.ppr;
	floatx16 acc;
#pragma unroll
	for (int r = 0; r < 16; r++) acc[r] = 0.f;
	for (int c0 = g_lo; c0 < g_hi; c0 += g.chunk_groups) { // (a chunk is at most QX_CHUNK_GROUPS groups: QX_UNROLL steps a wave)
		const int c1 = c0 + g.chunk_groups < g_hi ? c0 + g.chunk_groups : g_hi;
		const unsigned tile_block = qx_block_of(g, (unsigned)n0 * (unsigned)g.KG + (unsigned)c0);
		const unsigned base_block = g.dense ? tile_block : qx_block_of(g, row_g0 + (unsigned)c0);
		const int steps = (c1 - c0 + 1) >> 1; // an odd group count: the last step's upper half is zero
		unsigned long long bits[QX_UNROLL];
		int slot[QX_UNROLL];
		bool live[QX_UNROLL];
		halfx8 av[QX_UNROLL];
		// the chunk's index and activation loads first: they are in flight while the palettes are staged -- one round trip to memory per chunk, not two
#pragma unroll
		for (int u = 0; u < QX_UNROLL; u++) {
			const int t = wave + u * QX_WAVES, gi = c0 + 2 * t + hi;
			const bool in = t < steps && gi < c1;
			live[u] = in && row_ok;
			bits[u] = 0; slot[u] = 0;
#pragma unroll
			for (int e = 0; e < 8; e++) av[u][e] = (half_t)0.f;
			if (live[u]) {
				const unsigned G = row_g0 + (unsigned)gi, block = qx_block_of(g, G);
				const size_t off = (size_t)block * g.block_stride + (sizeof(half_t) << Q) + (size_t)(G - block * (unsigned)g.gpb) * Q;
				bits[u] = group_bits<Q>(g.w + off, 8, off + 8 <= g.in_len);
				slot[u] = (slot_base + (int)(block - base_block)) << Q;
			}
			if (in && a_ok) av[u] = *(const halfx8*)(a_row + 8 * (long)gi);
		}
		__syncthreads(); // the previous chunk's look-ups are done
		constexpr int VPP = 1 << (Q - 3); // 16-byte pieces of eight words per palette
		for (int i = tid; i < g.npal * VPP; i += QX_THREADS) {
			const int p = i >> (Q - 3);
			unsigned block;
			bool ok = true;
			if (g.dense) block = tile_block + (unsigned)p;
			else {
				const int r = (int)(((unsigned)p * g.ppr_m) >> 20); // p / ppr
				ok = n0 + r < g.N;
				block = qx_block_of(g, (unsigned)(n0 + r) * (unsigned)g.KG + (unsigned)c0) + (unsigned)(p - r * g.ppr);
			}
			if (ok && block < g.blocks) { // (every byte of an existing block's palette is inside the stream; its address may be odd)
				qx_u32x4 v;
				__builtin_memcpy(&v, g.w + (size_t)block * g.block_stride + 16 * (size_t)(i & (VPP - 1)), 16);
				*(qx_u32x4*)(lds + 16 * (size_t)i) = v;
			}
		}
		__syncthreads();
#pragma unroll
		for (int u = 0; u < QX_UNROLL; u++) {
			if (wave + u * QX_WAVES >= steps) break; // (the same for every lane of the wave)
			halfx8 wv;
#pragma unroll
			for (int e = 0; e < 8; e++) {
				const half_t v = pal[slot[u] + (int)((unsigned)(bits[u] >> (64 - Q * (e + 1))) & MASK)];
				wv[e] = live[u] ? v : (half_t)0.f; // (a lane without a group must supply zeros, not whatever slot 0 holds: 0 x inf)
			}
			acc = nnc_mfma_f16(av[u], wv, acc);
		}
	}
	__syncthreads(); // every look-up is done: the accumulators of waves 1 .. 3 take the palettes' place
	float* const red = (float*)lds; // [QX_WAVES - 1][16][64]
	if (wave > 0)
#pragma unroll
		for (int r = 0; r < 16; r++) red[((wave - 1) * 16 + r) * 64 + lane] = acc[r];
	__syncthreads();
	if (wave > 0 || !row_ok) return;
#pragma unroll
	for (int v = 0; v < QX_WAVES - 1; v++)
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

// b[m][n] = half(partial[0][m][n] + partial[1][m][n] + ... (in slice order) + bias[n])
__global__ void __launch_bounds__(256) gemm_qx_fold_kernel(const float* const partial, const int slices, const int M, const int N, const half_t* const bias, half_t* const b, const long ldb)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= M * N) return;
	const int m = i / N, n = i - m * N;
	float s = partial[i];
	for (int k = 1; k < slices; k++) s += partial[(size_t)k * (size_t)(M * N) + (size_t)i];
	if (bias) s += (float)bias[n];
	b[(long)m * ldb + n] = (half_t)s;
}

template <int Q>
static void gemm_qx_launch(const qx_geom_t& g, const int tiles, const int slices, hipStream_t stream)
{
	hipLaunchKernelGGL(HIP_KERNEL_NAME(gemm_qx_f16_kernel<Q>), dim3((unsigned)tiles, (unsigned)slices), dim3(QX_THREADS), 0, stream, g);
}

// The launch.  The caller has checked the operands (cmd_gemm.cpp gemm_qx_fused); here the geometry: slices, chunk, palette slots.  GEMM_QX_NOT_TAKEN: the palettes
// of two groups a chunk do not fit QX_LDS_BYTES, or the stream has 2^31 groups or more -- nothing was launched.
static int gemm_qx_f16_run(const unsigned char* const w, const int qbits, const int nib, const half_t* const a, const long lda, const half_t* const bias, half_t* const b, const long ldb, const int M, const int N, const int K, ccv_nnc_stream_context_t* const ctx)
{
	if ((double)N * (double)(K / 8) >= 2147483648.0) return GEMM_QX_NOT_TAKEN;
	qx_geom_t g;
	const size_t count = (size_t)N * (size_t)K;
	g.w = w; g.in_len = palettized_bytes(CCV_16F, count, qbits, nib);
	g.block_stride = (sizeof(half_t) << qbits) + index_bytes_per_block(qbits, nib);
	g.a = a; g.lda = lda; g.bias = bias; g.b = b; g.ldb = ldb; g.partial = 0;
	g.M = M; g.N = N; g.KG = K / 8; g.gpb = nib / 8;
	g.blocks = (unsigned)((count + (size_t)nib - 1) / (size_t)nib);
	int sh = 0;
	while ((1ll << sh) < g.gpb) sh++;
	g.div_sh = 31 + sh;
	g.div_m = (unsigned)(((1ull << g.div_sh) + (unsigned long long)g.gpb - 1) / (unsigned long long)g.gpb);
	const int tiles = (N + QX_TILE_N - 1) / QX_TILE_N;
	// slices: enough workgroups for four a CU, no slice shorter than QX_MIN_SLICE_GROUPS groups; the partials cost 8 M N bytes a slice, so no more than that
	long slices = tune(TUNE_GEMM_QX_SLICES);
	if (slices <= 0) {
		slices = (4l * device_cu_count() + tiles - 1) / tiles;
		if (slices > g.KG / QX_MIN_SLICE_GROUPS) slices = g.KG / QX_MIN_SLICE_GROUPS;
	}
	if (slices > g.KG) slices = g.KG;
	if (slices < 1) slices = 1;
	g.slice_groups = (int)(((g.KG + slices - 1) / slices + 1) & ~1l);
	slices = (g.KG + g.slice_groups - 1) / g.slice_groups;
	if (slices > 65535) return GEMM_QX_NOT_TAKEN;
	int cg = g.slice_groups < QX_CHUNK_GROUPS ? g.slice_groups : QX_CHUNK_GROUPS;
	for (;; cg = (cg / 2 + 1) & ~1) {
		const long len = 8l * cg;
		const long dense = ((long)(QX_TILE_N - 1) * K + len - 1) / nib + 2; // blocks from the tile's first row's first to its last row's last
		const long ppr = (len + nib - 9) / nib + 1;                        // blocks len consecutive elements starting at a multiple of eight touch, at most
		g.dense = dense <= ppr * QX_TILE_N;
		g.ppr = (int)ppr;
		g.ppr_m = (unsigned)(((1l << 20) + ppr - 1) / ppr); // exact: p (ppr_m ppr - 2^20) < 2048 * 32 < 2^20 for the slots 32 KiB hold
		const long npal = g.dense ? dense : ppr * QX_TILE_N;
		if ((npal * (long)sizeof(half_t)) << qbits <= QX_LDS_BYTES) { g.npal = (int)npal; break; }
		if (cg <= 2) return GEMM_QX_NOT_TAKEN;
	}
	g.chunk_groups = cg;
	hipStream_t stream = stream_of(ctx);
	if (slices > 1) {
		g.partial = (float*)workspace_of(ctx, sizeof(float) * (size_t)slices * (size_t)M * (size_t)N);
		if (!g.partial) return CCV_NNC_EXEC_OOM;
	}
	note_kernel("gemm_qx_f16");
	char prof_name[192];
	snprintf(prof_name, sizeof(prof_name), "gemm_fwd|nnc::gemm_qx_f16_kernel<%d> EPI = %s", qbits, slices <= 1 ? "EpiStoreH" : "EpiPartialH");
	{
		ProfScope prof(prof_name, 2.0 * (double)M * (double)N * (double)K, (double)g.in_len + 2.0 * ((double)M * K + (double)M * N), M, N, K, 1, (int)slices, stream);
		switch (qbits) {
			case 4: gemm_qx_launch<4>(g, tiles, (int)slices, stream); break;
			case 5: gemm_qx_launch<5>(g, tiles, (int)slices, stream); break;
			case 6: gemm_qx_launch<6>(g, tiles, (int)slices, stream); break;
			case 7: gemm_qx_launch<7>(g, tiles, (int)slices, stream); break;
			default: gemm_qx_launch<8>(g, tiles, (int)slices, stream); break;
		}
	}
	HIP_ENFORCE(hipGetLastError());
	if (slices > 1) {
		hipLaunchKernelGGL(gemm_qx_fold_kernel, dim3((unsigned)((M * N + 255) / 256)), dim3(256), 0, stream, (const float*)g.partial, (int)slices, M, N, bias, b, ldb);
		HIP_ENFORCE(hipGetLastError());
	}
	return CCV_NNC_EXEC_SUCCESS;
}

} // namespace nnc
