// SCALED_DOT_PRODUCT_ATTENTION backward on CCV_16F tensors for EVERY head size in 8s up to 256 (included by cmd_attention.cpp, inside its namespace, behind
// sdpa_anyd_f16.h).  sdpa_dq_f16_kernel / sdpa_dkv_f16_kernel take D and Dv in 32s up to 128; every other head size went through fp32 images and, there, the VALU
// kernels.  These kernels take D % 8 == 0, Dv % 8 == 0, 8 .. 256 each, with the forward any-D kernel's means:
//   padding inside    reductions over D / Dv run in whole 16-term steps of v_mfma_f32_32x32x16_f16: a 16-byte chunk past D (Dv) is zeros in the resident registers AND
//                     in the streamed tile; outputs are whole 32-column tiles whose 8-byte stores past D (Dv) are not issued; steps and tiles a shape does not need
//                     are skipped by wave-uniform tests (instances: D in 32s, Dv tiles in {1, 2, 3, 4, 6, 8})
//   one copy per tile every streamed tile lies in LDS AS IT LIES IN MEMORY ([row][width], one 16-byte store per chunk).  The products that reduce over the width read
//                     the lane's row (ds_read_b128); the products that reduce over the tile's ROWS assemble their A operand by two LDS transpose reads (isa.h
//                     tr_read4: rows 16 t + 4 half + 0..3 and + 8, sixteen columns of the tile).  Pitch: sdpa_anyd_vpitch -- 16 (mod 32) dwords, the four rows of
//                     a transpose-read block land 16 banks apart.  (sdpa_dq_f16_kernel / sdpa_dkv_f16_kernel keep a second, transposed copy written by eight
//                     2-byte stores per chunk.)
//   p, ds             stay in the registers they were computed in, rounded to half: the B operands of the second products (registers 8 t .. 8 t + 7 <-> the eight
//                     rows of sub-step t)
//   pipeline          ONE LDS buffer, the next block in REGISTERS: its global loads are issued right behind the barrier that published the current block
//   softmax factor    fp32, base 2: p = nnc_fast_exp2(s * (scale * log2 e) + (mask * log2 e - lse * log2 e)) -- one FMA on the score; lse * log2 e once per row
//   causal            a wave skips the products of a block none of its rows (dq) / none of whose rows (dk, dv) sees anything of; the barriers are kept
// dq:      a workgroup of four waves per (128 query rows, head, batch), a wave per 32 rows; q and g resident, K and V streamed in blocks of 32 keys.
//            S^T [keys x rows] = K Q^T, dP^T = V G^T (A = the lane's key row), dS^T = P^T o (dP^T - delta), dQ^T [D x rows] += K^T dS^T (A = transpose reads of K)
// dk, dv:  a workgroup per (128 keys, key head, batch), a wave per 32 keys; k (and v) resident, Q and G (and lse, delta) streamed in blocks of 32 rows, the Hq / Hk
//          query heads of the key head one after the other -- one fixed order of summation, no atomics.
//            S [rows x keys] = Q K^T, dP = G V^T (A = the lane's query row), dV^T [Dv x keys] += G^T P, dK^T [D x keys] += Q^T dS (A = transpose reads of G / Q)
//          Both gradients in one pass while D, Dv <= 192; above that one gradient per pass (registers: k 64 + v 64 + dK^T 128 + dV^T 128 at 256 / 256); the dv pass
//          needs k, S and G only.
#pragma once

// acc[i] += (tile^T) b for the output tiles i < n: A = columns 32 i + (l & 31) of the tile rows 16 tt + 4 lh + 0..3 and + 8 (blk = that row, column 16 (li >> 4)), four
// tiles per wait: the transpose reads are asm, hipcc does not count them
template <int T>
__device__ __forceinline__ void sdpa_bwd_tr_products(floatx16 (&acc)[T], const int n, const half_t* const blk, const int pitch, const int li, const halfx8 b)
{
#pragma unroll
	for (int t0 = 0; t0 < T; t0 += 4) {
		if (t0 >= n) break;
		halfx4 lo[4], hi[4];
#pragma unroll
		for (int u = 0; u < 4; u++)
			if (t0 + u < T) { lo[u] = tr_read4(blk + 32 * (t0 + u), pitch, li & 15); hi[u] = tr_read4(blk + 32 * (t0 + u) + 8 * pitch, pitch, li & 15); }
		NNC_WAIT_LGKM0();
#pragma unroll
		for (int u = 0; u < 4; u++)
			if (t0 + u < T) { NNC_PIN_VEC(lo[u]); NNC_PIN_VEC(hi[u]); }
#pragma unroll
		for (int u = 0; u < 4; u++)
			if (t0 + u < T) {
				if (t0 + u < n) acc[t0 + u] = nnc_mfma_f16(halfx8{ lo[u][0], lo[u][1], lo[u][2], lo[u][3], hi[u][0], hi[u][1], hi[u][2], hi[u][3] }, b, acc[t0 + u]);
			}
	}
}

template <int DS, int TV> // DS (even) >= ceil(D / 16), TV >= ceil(Dv / 32): the LDS and register layout; steps and tiles past D / Dv are skipped (wave-uniform)
__global__ void __launch_bounds__(256) sdpa_bwd_anyd_dq_f16_kernel(const sdpa_geom_t g, const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, const half_t* __restrict__ mask, const half_t* __restrict__ gr, const long g_sb, const long g_sr, const long g_sh, const float* __restrict__ lse, const float* __restrict__ delta, half_t* __restrict__ dq, const long dq_sb, const long dq_sr, const long dq_sh)
{
	constexpr int TD = DS / 2, GS = 2 * TV, KP = sdpa_anyd_vpitch<TD>(), VP = sdpa_anyd_vpitch<TV>();
	constexpr int KCH = 4 * TD, VCH = 4 * TV; // 16-byte chunks per key row of the tiles
	constexpr int NK = (32 * KCH + 255) / 256, NV = (32 * VCH + 255) / 256; // chunks per lane and block
	__shared__ __attribute__((aligned(16))) half_t Ks[32 * KP];
	__shared__ __attribute__((aligned(16))) half_t Vs[32 * VP];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int li = lane & 31, lh = lane >> 5;
	const int h = blockIdx.y, b = blockIdx.z, hk = h / g.ratio;
	const int x = blockIdx.x * 128 + wave * 32 + li;
	const int ds_n = (g.D + 15) >> 4, gs_n = (g.Dv + 15) >> 4, td_n = (g.D + 31) >> 5;
	const halfx8 zero8 = halfx8{ 0, 0, 0, 0, 0, 0, 0, 0 };
	halfx8 qf[DS], gf[GS];
#pragma unroll
	for (int s = 0; s < DS; s++) {
		qf[s] = zero8;
		if (x < g.R && 16 * s + 8 * lh < g.D) qf[s] = *(const halfx8*)(q + b * g.q_sb + (long)x * g.q_sr + h * g.q_sh + 16 * s + 8 * lh);
	}
#pragma unroll
	for (int s = 0; s < GS; s++) {
		gf[s] = zero8;
		if (x < g.R && 16 * s + 8 * lh < g.Dv) gf[s] = *(const halfx8*)(gr + b * g_sb + (long)x * g_sr + h * g_sh + 16 * s + 8 * lh);
	}
	floatx16 acc[TD];
#pragma unroll
	for (int td = 0; td < TD; td++)
#pragma unroll
		for (int r = 0; r < 16; r++) acc[td][r] = 0.f;
	const int vis = x < g.R ? visible_keys(g, x) : 0;
	int vis_wg, vis_wave = 0; // keys the workgroup's / the wave's last row sees: visible_keys() does not fall with x
	{
		const int x_wg = blockIdx.x * 128 + 127 < g.R ? blockIdx.x * 128 + 127 : g.R - 1;
		vis_wg = visible_keys(g, x_wg);
		const int xw0 = blockIdx.x * 128 + wave * 32;
		if (xw0 < g.R) vis_wave = visible_keys(g, xw0 + 31 < g.R ? xw0 + 31 : g.R - 1);
	}
	const float LOG2E = 1.4426950408889634f;
	const float c2 = g.scale * LOG2E;
	// a row that sees no key has lse = -inf and vis = 0: none of its terms is evaluated
	const float lse2 = vis > 0 ? lse[((long)b * g.Hq + h) * g.R + x] * LOG2E : 0.f, my_delta = vis > 0 ? delta[((long)b * g.Hq + h) * g.R + x] : 0.f;
	const half_t* const mrow = mask ? mask + b * g.m_sb + h * g.m_sh + (long)(x < g.R ? x : 0) * g.m_sr : 0;
	const half_t* const kbase = k + b * g.k_sb + hk * g.k_sh;
	const half_t* const vbase = v + b * g.v_sb + hk * g.v_sh;
	halfx8 kr[NK], vr[NV];
	if (vis_wg > 0) SDPA_ANYD_FETCH(0); // (sdpa_anyd_f16.h)
	for (int y0 = 0; y0 < vis_wg; y0 += 32) {
		__syncthreads(); // every wave is done with the tiles of the block before
#pragma unroll
		for (int jj = 0; jj < NK; jj++) {
			const int c = t + 256 * jj, j = c / KCH, d = (c - j * KCH) << 3;
			if (c < 32 * KCH) *(halfx8*)(Ks + j * KP + d) = kr[jj]; // as it lies: one 16-byte store per chunk
		}
#pragma unroll
		for (int jj = 0; jj < NV; jj++) {
			const int c = t + 256 * jj, j = c / VCH, d = (c - j * VCH) << 3;
			if (c < 32 * VCH) *(halfx8*)(Vs + j * VP + d) = vr[jj];
		}
		__syncthreads();
		if (y0 + 32 < vis_wg) SDPA_ANYD_FETCH(y0 + 32); // in flight while this block is computed
		if (y0 >= vis_wave) continue; // none of the wave's rows sees a key of this block (the barriers above are passed by every wave all the same)
		floatx16 s, dp;
#pragma unroll
		for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
		for (int i = 0; i < DS; i++)
			if (i < ds_n) s = nnc_mfma_f16(*(const halfx8*)(Ks + li * KP + 16 * i + 8 * lh), qf[i], s);
#pragma unroll
		for (int i = 0; i < GS; i++)
			if (i < gs_n) dp = nnc_mfma_f16(*(const halfx8*)(Vs + li * VP + 16 * i + 8 * lh), gf[i], dp);
		// this lane's row: register r <-> key y0 + (r & 3) + 8 (r >> 2) + 4 lh; s becomes ds
#pragma unroll
		for (int r = 0; r < 16; r++) {
			const int y = y0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
			float e = 0.f;
			if (y < vis) e = nnc_fast_exp2(fmaf(s[r], c2, mrow ? fmaf((float)mrow[y], LOG2E, -lse2) : -lse2)) * (dp[r] - my_delta);
			s[r] = e;
		}
#pragma unroll
		for (int tt = 0; tt < 2; tt++)
			sdpa_bwd_tr_products<TD>(acc, td_n, Ks + (16 * tt + 4 * lh) * KP + 16 * (li >> 4), KP, li, sdpa_half8(s, tt));
	}
#undef SDPA_ANYD_FETCH
	if (x < g.R) {
		half_t* const orow = dq + b * dq_sb + (long)x * dq_sr + h * dq_sh;
#pragma unroll
		for (int td = 0; td < TD; td++)
#pragma unroll
			for (int r4 = 0; r4 < 4; r4++) { // registers 4 r4 .. 4 r4 + 3 are d = 32 td + 8 r4 + 4 lh + 0..3
				const int d = 32 * td + 8 * r4 + 4 * lh;
				if (d < g.D) *(halfx4*)(orow + d) = halfx4{ (half_t)(g.scale * acc[td][4 * r4]), (half_t)(g.scale * acc[td][4 * r4 + 1]), (half_t)(g.scale * acc[td][4 * r4 + 2]), (half_t)(g.scale * acc[td][4 * r4 + 3]) };
			}
	}
}

template <int DS, int TV, bool DO_K, bool DO_V> // as above; DO_K / DO_V: the gradients this instance can produce (a null dk / dv skips its products at run time)
__global__ void __launch_bounds__(256) sdpa_bwd_anyd_dkv_f16_kernel(const sdpa_geom_t g, const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, const half_t* __restrict__ mask, const half_t* __restrict__ gr, const long g_sb, const long g_sr, const long g_sh, const float* __restrict__ lse, const float* __restrict__ delta, half_t* __restrict__ dk, const long dk_sb, const long dk_sc, const long dk_sh, half_t* __restrict__ dv, const long dv_sb, const long dv_sc, const long dv_sh)
{
	constexpr int TD = DS / 2, GS = 2 * TV, QP = sdpa_anyd_vpitch<TD>(), GP = sdpa_anyd_vpitch<TV>();
	constexpr int QCH = 4 * TD, GCH = 4 * TV; // 16-byte chunks per query row of the tiles
	constexpr int NQ = (32 * QCH + 255) / 256, NG = (32 * GCH + 255) / 256; // chunks per lane and block
	constexpr int NAK = DO_K ? TD : 1, NAV = DO_V ? TV : 1, NVF = DO_K ? GS : 1;
	__shared__ __attribute__((aligned(16))) half_t Qs[32 * QP];
	__shared__ __attribute__((aligned(16))) half_t Gs[32 * GP];
	__shared__ float Ls[32], Dl[32]; // lse * log2 e and delta of the block's rows
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int li = lane & 31, lh = lane >> 5;
	const int hk = blockIdx.y, b = blockIdx.z;
	const int y0wg = blockIdx.x * 128, y0wave = y0wg + wave * 32, y = y0wave + li;
	const int ds_n = (g.D + 15) >> 4, gs_n = (g.Dv + 15) >> 4, td_n = (g.D + 31) >> 5, tv_n = (g.Dv + 31) >> 5;
	const bool want_k = DO_K && dk, want_v = DO_V && dv;
	const halfx8 zero8 = halfx8{ 0, 0, 0, 0, 0, 0, 0, 0 };
	halfx8 kf[DS], vf[NVF];
#pragma unroll
	for (int s = 0; s < DS; s++) {
		kf[s] = zero8;
		if (y < g.C && 16 * s + 8 * lh < g.D) kf[s] = *(const halfx8*)(k + b * g.k_sb + (long)y * g.k_sc + hk * g.k_sh + 16 * s + 8 * lh);
	}
	if (DO_K) {
#pragma unroll
		for (int s = 0; s < NVF; s++) {
			vf[s] = zero8;
			if (y < g.C && 16 * s + 8 * lh < g.Dv) vf[s] = *(const halfx8*)(v + b * g.v_sb + (long)y * g.v_sc + hk * g.v_sh + 16 * s + 8 * lh);
		}
	}
	floatx16 ak[NAK], av[NAV];
#pragma unroll
	for (int i = 0; i < NAK; i++)
#pragma unroll
		for (int r = 0; r < 16; r++) ak[i][r] = 0.f;
#pragma unroll
	for (int i = 0; i < NAV; i++)
#pragma unroll
		for (int r = 0; r < 16; r++) av[i][r] = 0.f;
	// key y is seen by the rows x >= y + R - C (causal): the first query block of the workgroup / the first row that sees anything of the wave
	int xs = 0, xs_wave = 0;
	if (g.causal) {
		xs = y0wg + g.R - g.C; if (xs < 0) xs = 0; xs = xs / 32 * 32;
		xs_wave = y0wave + g.R - g.C; if (xs_wave < 0) xs_wave = 0;
	}
	const bool wave_live = y0wave < g.C;
	const int nblk = xs < g.R ? (g.R - xs + 31) / 32 : 0, nit = nblk * g.ratio; // query blocks per head; the heads of this key head one after the other
	const float LOG2E = 1.4426950408889634f;
	const float c2 = g.scale * LOG2E;
	halfx8 qr[NQ], gg[NG];
	float lr = 0.f, dr = 0.f;
	// the lane's chunks of block `it`: head hk * ratio + it / nblk, rows xs + 32 (it % nblk) ..; past R, past D / Dv: zeros.  Lanes 0 .. 31 of wave 0: lse, delta
#define SDPA_BWD_DKV_FETCH(it) do { \
		const int fh = hk * g.ratio + (it) / nblk, fx = xs + 32 * ((it) % nblk); \
		const half_t* const qbase = q + b * g.q_sb + fh * g.q_sh; \
		const half_t* const gbase = gr + b * g_sb + fh * g_sh; \
		_Pragma("unroll") for (int jj = 0; jj < NQ; jj++) { \
			const int c = t + 256 * jj, j = c / QCH, d = (c - j * QCH) << 3; \
			qr[jj] = zero8; \
			if (c < 32 * QCH && fx + j < g.R && d < g.D) qr[jj] = *(const halfx8*)(qbase + (long)(fx + j) * g.q_sr + d); \
		} \
		_Pragma("unroll") for (int jj = 0; jj < NG; jj++) { \
			const int c = t + 256 * jj, j = c / GCH, d = (c - j * GCH) << 3; \
			gg[jj] = zero8; \
			if (c < 32 * GCH && fx + j < g.R && d < g.Dv) gg[jj] = *(const halfx8*)(gbase + (long)(fx + j) * g_sr + d); \
		} \
		lr = 0.f; dr = 0.f; \
		if (t < 32 && fx + t < g.R) { lr = lse[((long)b * g.Hq + fh) * g.R + fx + t] * LOG2E; dr = delta[((long)b * g.Hq + fh) * g.R + fx + t]; } } while (0)
	if (nit > 0) SDPA_BWD_DKV_FETCH(0);
	for (int it = 0; it < nit; it++) {
		const int h = hk * g.ratio + it / nblk, x0 = xs + 32 * (it % nblk);
		__syncthreads(); // every wave is done with the tiles of the block before
#pragma unroll
		for (int jj = 0; jj < NQ; jj++) {
			const int c = t + 256 * jj, j = c / QCH, d = (c - j * QCH) << 3;
			if (c < 32 * QCH) *(halfx8*)(Qs + j * QP + d) = qr[jj]; // as it lies: one 16-byte store per chunk
		}
#pragma unroll
		for (int jj = 0; jj < NG; jj++) {
			const int c = t + 256 * jj, j = c / GCH, d = (c - j * GCH) << 3;
			if (c < 32 * GCH) *(halfx8*)(Gs + j * GP + d) = gg[jj];
		}
		if (t < 32) { Ls[t] = lr; Dl[t] = dr; }
		__syncthreads();
		if (it + 1 < nit) SDPA_BWD_DKV_FETCH(it + 1); // in flight while this block is computed
		if (!wave_live || x0 + 32 <= xs_wave) continue; // no row of this block sees a key of the wave (the barriers above are passed by every wave all the same)
		floatx16 s, dp;
#pragma unroll
		for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
		for (int i = 0; i < DS; i++)
			if (i < ds_n) s = nnc_mfma_f16(*(const halfx8*)(Qs + li * QP + 16 * i + 8 * lh), kf[i], s);
		if (want_k) {
#pragma unroll
			for (int i = 0; i < NVF; i++)
				if (i < gs_n) dp = nnc_mfma_f16(*(const halfx8*)(Gs + li * GP + 16 * i + 8 * lh), vf[i], dp);
		}
		// this lane's key: register r <-> row x0 + (r & 3) + 8 (r >> 2) + 4 lh; s becomes p, dp becomes ds
#pragma unroll
		for (int r = 0; r < 16; r++) {
			const int qx = (r & 3) + 8 * (r >> 2) + 4 * lh, x = x0 + qx;
			float p = 0.f;
			if (x < g.R && y < g.C && y < visible_keys(g, x)) p = nnc_fast_exp2(fmaf(s[r], c2, mask ? fmaf((float)mask[b * g.m_sb + h * g.m_sh + (long)x * g.m_sr + y], LOG2E, -Ls[qx]) : -Ls[qx]));
			s[r] = p;
			dp[r] = p * (dp[r] - Dl[qx]);
		}
#pragma unroll
		for (int tt = 0; tt < 2; tt++) {
			if (want_v) sdpa_bwd_tr_products<NAV>(av, tv_n, Gs + (16 * tt + 4 * lh) * GP + 16 * (li >> 4), GP, li, sdpa_half8(s, tt));
			if (want_k) sdpa_bwd_tr_products<NAK>(ak, td_n, Qs + (16 * tt + 4 * lh) * QP + 16 * (li >> 4), QP, li, sdpa_half8(dp, tt));
		}
	}
#undef SDPA_BWD_DKV_FETCH
	if (y < g.C) {
#pragma unroll
		for (int r4 = 0; r4 < 4; r4++) { // registers 4 r4 .. 4 r4 + 3 of tile i are column 32 i + 8 r4 + 4 lh + 0..3 of this lane's key
			if (want_k) {
				half_t* const o = dk + b * dk_sb + (long)y * dk_sc + hk * dk_sh;
#pragma unroll
				for (int i = 0; i < NAK; i++) {
					const int d = 32 * i + 8 * r4 + 4 * lh;
					if (d < g.D) *(halfx4*)(o + d) = halfx4{ (half_t)(g.scale * ak[i][4 * r4]), (half_t)(g.scale * ak[i][4 * r4 + 1]), (half_t)(g.scale * ak[i][4 * r4 + 2]), (half_t)(g.scale * ak[i][4 * r4 + 3]) };
				}
			}
			if (want_v) {
				half_t* const o = dv + b * dv_sb + (long)y * dv_sc + hk * dv_sh;
#pragma unroll
				for (int i = 0; i < NAV; i++) {
					const int d = 32 * i + 8 * r4 + 4 * lh;
					if (d < g.Dv) *(halfx4*)(o + d) = halfx4{ (half_t)av[i][4 * r4], (half_t)av[i][4 * r4 + 1], (half_t)av[i][4 * r4 + 2], (half_t)av[i][4 * r4 + 3] };
				}
			}
		}
	}
}

// D % 8 == 0, Dv % 8 == 0, 8 <= D, Dv <= 256; 16-byte aligned q / k / v / g rows, 8-byte aligned dq / dk / dv rows (the caller checks); lse, delta: the forward
// re-run's log-sum-exp and sdpa_delta_h_kernel's row sums
static void sdpa_bwd_anyd_f16_launch(const sdpa_geom_t& g, const sdpa_back_ops_t& a, hipStream_t stream)
{
	const int ds = (g.D + 15) / 16, tv = (g.Dv + 31) / 32;
	half_t* const dqp = (half_t*)a.dq.p; half_t* const dkp = (half_t*)a.dk.p; half_t* const dvp = (half_t*)a.dv.p;
	if (dqp) {
		const dim3 grid((g.R + 127) / 128, g.Hq, g.B);
		note_kernel("sdpa_bwd_anyd_dq_f16");
		ProfScope prof("sdpa_bwd_dq_h_anyd|nnc::sdpa_bwd_anyd_dq_f16_kernel", 2.0 * g.B * g.Hq * (double)g.R * g.C * (2 * g.D + g.Dv), 0, g.R, g.C, g.D, g.B * g.Hq, 1, stream);
		sdpa_pick(sdpa_anyd_ds(), ds, sdpa_anyd_tv(), tv, [&](auto s, auto t) { sdpa_launch_dq<half_t>(sdpa_bwd_anyd_dq_f16_kernel<decltype(s)::value, decltype(t)::value>, grid, stream, g, a); });
		HIP_ENFORCE(hipGetLastError());
	}
	if (dkp || dvp) {
		const dim3 grid((g.C + 127) / 128, g.Hk, g.B);
		note_kernel("sdpa_bwd_anyd_dkv_f16");
		if (ds <= 12 && tv <= 6) { // both gradients in one pass
			ProfScope prof("sdpa_bwd_dkv_h_anyd|nnc::sdpa_bwd_anyd_dkv_f16_kernel", 2.0 * g.B * g.Hq * (double)g.R * g.C * ((dkp ? 2 * g.D + g.Dv : g.D) + (dvp ? g.Dv : 0)), 0, g.C, g.R, g.D, g.B * g.Hk, 1, stream);
			sdpa_pick(sdpa_ints<2, 4, 6, 8, 10, 12>(), ds, sdpa_ints<1, 2, 3, 4, 6>(), tv, [&](auto s, auto t) {
				sdpa_launch_dkv<half_t>(sdpa_bwd_anyd_dkv_f16_kernel<decltype(s)::value, decltype(t)::value, true, true>, grid, stream, g, a); });
			HIP_ENFORCE(hipGetLastError());
		} else { // one gradient per pass (registers): dv first, then dk.  Only the instances this branch can reach are compiled: D > 192 with any Dv, or Dv > 192
			const auto pass = [&](auto do_k, auto do_v) {
				constexpr bool DO_K = decltype(do_k)::value, DO_V = decltype(do_v)::value;
				if (ds > 12) sdpa_pick(sdpa_ints<14, 16>(), ds, sdpa_anyd_tv(), tv, [&](auto s, auto t) { sdpa_launch_dkv<half_t>(sdpa_bwd_anyd_dkv_f16_kernel<decltype(s)::value, decltype(t)::value, DO_K, DO_V>, grid, stream, g, a); });
				else sdpa_pick(sdpa_ints<2, 4, 6, 8, 10, 12>(), ds, [&](auto s) { sdpa_launch_dkv<half_t>(sdpa_bwd_anyd_dkv_f16_kernel<decltype(s)::value, 8, DO_K, DO_V>, grid, stream, g, a); });
				HIP_ENFORCE(hipGetLastError());
			};
			if (dvp) {
				ProfScope prof("sdpa_bwd_dv_h_anyd|nnc::sdpa_bwd_anyd_dkv_f16_kernel", 2.0 * g.B * g.Hq * (double)g.R * g.C * (g.D + g.Dv), 0, g.C, g.R, g.D, g.B * g.Hk, 1, stream);
				pass(std::false_type(), std::true_type());
			}
			if (dkp) {
				ProfScope prof("sdpa_bwd_dk_h_anyd|nnc::sdpa_bwd_anyd_dkv_f16_kernel", 2.0 * g.B * g.Hq * (double)g.R * g.C * (2 * g.D + g.Dv), 0, g.C, g.R, g.D, g.B * g.Hk, 1, stream);
				pass(std::true_type(), std::false_type());
			}
		}
	}
}
