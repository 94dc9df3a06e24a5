// SCALED_DOT_PRODUCT_ATTENTION forward on CCV_16F tensors for EVERY head size in 8s up to 256 (included by cmd_attention.cpp, inside its namespace, behind
// sdpa_geom_t and visible_keys).  The f16 kernel of round 4 (sdpa_forw_f16_kernel) takes D in 16s and Dv in 32s up to 128; the heads of the diffusion U-Nets
// (40, 80, 160) and of current transformers (72, 192, 256) went through fp32 images.  This kernel takes D % 8 == 0, Dv % 8 == 0, 8 .. 256 each, and pads
// INSIDE -- never in memory:
//   reduction   rounded up to whole 16-term steps of v_mfma_f32_32x32x16_f16: a 16-byte chunk past D is zeros in the q registers AND in the K tile
//   output      rounded up to whole 32-column tiles: V chunks past Dv are zeros in the V tile, their 8-byte stores are not issued (Dv % 8 == 0: a store of four
//               halves lies wholly inside or wholly outside)
// Work split: a workgroup of four waves per (128 query rows, head, batch), a wave per 32 rows, key blocks of 32.  Per block and wave
//   S^T [32 keys x 32 rows] = K Q^T    A = ds_read_b128 of the lane's key row out of the K tile ([key][16 DS + 8 halves]), B = the lane's q chunk, in registers for
//                                      the whole kernel; lane (l & 31, half l >> 5) stands for d = 16 s + 8 half + 0..7 in both operands
//   O^T [Dv x 32 rows] += V^T P^T      two sub-steps of 16 keys.  B = the probabilities in the registers they were computed in: the lane holds keys
//                                      ky(r) = (r & 3) + 8 (r >> 2) + 4 half of its row, sub-step t is registers 8 t .. 8 t + 7 rounded to half.  A = the same eight
//                                      keys of column dv = l & 31: V lies in LDS AS IT LIES IN MEMORY ([key][Dv], one 16-byte store per chunk) and the operand is
//                                      assembled by two LDS transpose reads (isa.h tr_read4: rows = keys 16 t + 4 half + 0..3 and + 8, columns = 16 dv of the tile).
//                                      (sdpa_forw_f16_kernel transposes on the way in: eight 2-byte LDS stores per chunk.)
// The V tile's pitch is 32 TV halves for odd TV and 32 TV + 32 for even TV: 16 (mod 32) dwords, so the four key rows of a transpose-read block land 16 banks apart
// (mfma_gemm_f16.h gemm16_npitch's arithmetic).  The K tile's pitch is 16 DS + 8 halves (4 mod 8 dwords: the 16-byte fragment reads of a 16-lane group do not collide).
// D = Dv = 256: 32 x 264 + 32 x 288 halves = 35,328 bytes of LDS.
// Pipeline: ONE LDS buffer, the next block in REGISTERS: the global loads of block y0 + 32 are issued right behind the barrier that published block y0, in front of
// its MFMAs, and stored to LDS behind the barrier that ends block y0 (DS / 4 + TV / 2 chunks per lane: 32 registers at 256 / 256 beside 64 of q, 128 of O^T, 16 of S^T).
// Softmax in fp32 in the base-2 domain: u = s * (scale * log2 e) + mask * log2 e in one FMA, p = nnc_fast_exp2(u - m); running maximum and sum per row as in the
// other forward kernels; a row that sees no key gives 0 and -inf.  A wave whose 32 rows see nothing of a key block (the causal triangle) skips its products.
// Instances: DS in 2s (one step is skipped at run time where D needs one fewer), TV in {1, 2, 3, 4, 6, 8} (tiles past Dv are skipped at run time).
#pragma once

template <int TV> constexpr int sdpa_anyd_vpitch() { return 32 * TV + (TV % 2 ? 0 : 32); }
// the instances of this file's kernel and of sdpa_anyd_f16_back.h's: 16-term steps over D in 2s, 32-column tiles of Dv
using sdpa_anyd_ds = sdpa_ints<2, 4, 6, 8, 10, 12, 14, 16>;
using sdpa_anyd_tv = sdpa_ints<1, 2, 3, 4, 6, 8>;
// The lane's chunks of the key block at y, into its registers kr[NK] / vr[NV] (this file's kernel and the dq kernel of sdpa_anyd_f16_back.h: K tile rows of KCH
// chunks off kbase, V tile rows of VCH chunks off vbase): chunk c = t + 256 jj is key c / KCH (c / VCH), halves 8 (c % KCH) .. + 7; past C, past D / Dv: zeros
#define SDPA_ANYD_FETCH(y) do { \
		_Pragma("unroll") for (int jj = 0; jj < NK; jj++) { \
			const int c = t + 256 * jj, j = c / KCH, d = (c - j * KCH) << 3; \
			kr[jj] = zero8; \
			if (c < 32 * KCH && (y) + j < g.C && d < g.D) kr[jj] = *(const halfx8*)(kbase + (long)((y) + j) * g.k_sc + d); \
		} \
		_Pragma("unroll") for (int jj = 0; jj < NV; jj++) { \
			const int c = t + 256 * jj, j = c / VCH, d = (c - j * VCH) << 3; \
			vr[jj] = zero8; \
			if (c < 32 * VCH && (y) + j < g.C && d < g.Dv) vr[jj] = *(const halfx8*)(vbase + (long)((y) + j) * g.v_sc + d); \
		} } while (0)

template <int DS, int TV> // DS >= ceil(D / 16), TV >= ceil(Dv / 32): the LDS and register layout; the steps and tiles past D / Dv are skipped (wave-uniform)
__global__ void __launch_bounds__(256) sdpa_fwd_anyd_f16_kernel(const sdpa_geom_t g, const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, const half_t* __restrict__ mask, half_t* __restrict__ o, float* __restrict__ lse)
{
	constexpr int KP = 16 * DS + 8, VP = sdpa_anyd_vpitch<TV>();
	constexpr int KCH = 2 * DS, VCH = 4 * TV; // 16-byte chunks per key row of the tiles
	constexpr int NK = (32 * KCH + 255) / 256, NV = (32 * VCH + 255) / 256; // chunks per lane and block
	__shared__ __attribute__((aligned(16))) half_t Ks[32 * KP];
	__shared__ __attribute__((aligned(16))) half_t Vs[32 * VP];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int li = lane & 31, lh = lane >> 5;
	const int h = blockIdx.y, b = blockIdx.z, hk = h / g.ratio;
	const int x = blockIdx.x * 128 + wave * 32 + li;
	const int ds_n = (g.D + 15) >> 4, tv_n = (g.Dv + 31) >> 5;
	const halfx8 zero8 = halfx8{ 0, 0, 0, 0, 0, 0, 0, 0 };
	halfx8 qf[DS];
#pragma unroll
	for (int s = 0; s < DS; s++) {
		qf[s] = zero8;
		if (x < g.R && 16 * s + 8 * lh < g.D) qf[s] = *(const halfx8*)(q + b * g.q_sb + (long)x * g.q_sr + h * g.q_sh + 16 * s + 8 * lh);
	}
	floatx16 acc[TV];
#pragma unroll
	for (int tv = 0; tv < TV; tv++)
#pragma unroll
		for (int r = 0; r < 16; r++) acc[tv][r] = 0.f;
	float m_run = -INFINITY, l_run = 0.f; // base-2 domain
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
	const half_t* const mrow = mask ? mask + b * g.m_sb + h * g.m_sh + (long)(x < g.R ? x : 0) * g.m_sr : 0;
	const half_t* const kbase = k + b * g.k_sb + hk * g.k_sh;
	const half_t* const vbase = v + b * g.v_sb + hk * g.v_sh;
	halfx8 kr[NK], vr[NV];
	if (vis_wg > 0) SDPA_ANYD_FETCH(0);
	for (int y0 = 0; y0 < vis_wg; y0 += 32) {
		__syncthreads(); // every wave is done with the tiles of the block before
#pragma unroll
		for (int jj = 0; jj < NK; jj++) {
			const int c = t + 256 * jj, j = c / KCH, d = (c - j * KCH) << 3;
			if (c < 32 * KCH) *(halfx8*)(Ks + j * KP + d) = kr[jj];
		}
#pragma unroll
		for (int jj = 0; jj < NV; jj++) {
			const int c = t + 256 * jj, j = c / VCH, d = (c - j * VCH) << 3;
			if (c < 32 * VCH) *(halfx8*)(Vs + j * VP + d) = vr[jj]; // as it lies: one 16-byte store per chunk
		}
		__syncthreads();
		if (y0 + 32 < vis_wg) SDPA_ANYD_FETCH(y0 + 32); // in flight while this block is computed
		if (y0 >= vis_wave) continue; // none of the wave's rows sees a key of this block (the barriers above are passed by every wave all the same)
		floatx16 s;
#pragma unroll
		for (int r = 0; r < 16; r++) s[r] = 0.f;
#pragma unroll
		for (int i = 0; i < DS; i++)
			if (i < ds_n) s = nnc_mfma_f16(*(const halfx8*)(Ks + li * KP + 16 * i + 8 * lh), qf[i], s);
		// scores of this lane's row: register r <-> key y0 + (r & 3) + 8 (r >> 2) + 4 lh
		float bm = -INFINITY;
#pragma unroll
		for (int r = 0; r < 16; r++) {
			const int y = y0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
			if (y < vis) { s[r] = mrow ? fmaf(s[r], c2, (float)mrow[y] * LOG2E) : s[r] * c2; bm = fmaxf(bm, s[r]); }
			else s[r] = -INFINITY;
		}
		bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
		const float m_new = fmaxf(m_run, bm);
		const float m_sub = m_new == -INFINITY ? 0.f : m_new; // (a row that has seen nothing yet, or -inf masks only: every term below is exp2(-inf) = 0)
		float ps = 0.f;
#pragma unroll
		for (int r = 0; r < 16; r++) {
			s[r] = nnc_fast_exp2(s[r] - m_sub);
			ps += s[r];
		}
		ps += __shfl_xor(ps, 32, 64);
		const float alpha = nnc_fast_exp2(m_run - m_sub);
		l_run = l_run * alpha + ps;
		m_run = m_new;
#pragma unroll
		for (int tv = 0; tv < TV; tv++)
			if (tv < tv_n)
#pragma unroll
				for (int r = 0; r < 16; r++) acc[tv][r] *= alpha;
#pragma unroll
		for (int tt = 0; tt < 2; tt++) { // (sdpa_anyd_f16_back.h's sdpa_bwd_tr_products written out: through the helper 40 instances of this kernel compile differently)
			const halfx8 pf = sdpa_half8(s, tt);
			const half_t* const blk = Vs + (16 * tt + 4 * lh) * VP + 16 * (li >> 4);
#pragma unroll
			for (int t0 = 0; t0 < TV; t0 += 4) { // four output tiles per wait: the transpose reads are asm, hipcc does not count them
				if (t0 >= tv_n) break;
				halfx4 lo[4], hi[4];
#pragma unroll
				for (int u = 0; u < 4; u++)
					if (t0 + u < TV) { lo[u] = tr_read4(blk + 32 * (t0 + u), VP, li & 15); hi[u] = tr_read4(blk + 32 * (t0 + u) + 8 * VP, VP, li & 15); }
				NNC_WAIT_LGKM0();
#pragma unroll
				for (int u = 0; u < 4; u++)
					if (t0 + u < TV) { NNC_PIN_VEC(lo[u]); NNC_PIN_VEC(hi[u]); }
#pragma unroll
				for (int u = 0; u < 4; u++)
					if (t0 + u < TV) {
						if (t0 + u < tv_n) acc[t0 + u] = nnc_mfma_f16(halfx8{ lo[u][0], lo[u][1], lo[u][2], lo[u][3], hi[u][0], hi[u][1], hi[u][2], hi[u][3] }, pf, acc[t0 + u]);
					}
			}
		}
	}
	if (x < g.R) {
		const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
		half_t* const orow = o + b * g.o_sb + (long)x * g.o_sr + h * g.o_sh;
#pragma unroll
		for (int tv = 0; tv < TV; tv++)
#pragma unroll
			for (int r4 = 0; r4 < 4; r4++) { // registers 4 r4 .. 4 r4 + 3 are dv = 32 tv + 8 r4 + 4 lh + 0..3
				const int dv = 32 * tv + 8 * r4 + 4 * lh;
				if (dv < g.Dv) *(halfx4*)(orow + dv) = halfx4{ (half_t)(acc[tv][4 * r4] * inv), (half_t)(acc[tv][4 * r4 + 1] * inv), (half_t)(acc[tv][4 * r4 + 2] * inv), (half_t)(acc[tv][4 * r4 + 3] * inv) };
			}
		if (lse && lh == 0) lse[((long)b * g.Hq + h) * g.R + x] = l_run > 0.f ? (m_run + log2f(l_run)) * 0.6931471805599453f : -INFINITY;
	}
}

// D % 8 == 0, Dv % 8 == 0, 8 <= D, Dv <= 256; 16-byte aligned q / k / v rows, 8-byte aligned o rows (the caller checks)
static void sdpa_fwd_anyd_f16_launch(const sdpa_geom_t& g, const half_t* const qp, const half_t* const kp, const half_t* const vp, const half_t* const mp, half_t* const op, float* const lse, hipStream_t stream)
{
	const dim3 grid((g.R + 127) / 128, g.Hq, g.B);
	note_kernel("sdpa_fwd_anyd_f16");
	ProfScope prof("sdpa_fwd_h_anyd|nnc::sdpa_fwd_anyd_f16_kernel", 2.0 * g.B * g.Hq * (double)g.R * g.C * (g.D + g.Dv), 0, g.R, g.C, g.D, g.B * g.Hq, 1, stream);
	sdpa_pick(sdpa_anyd_ds(), (g.D + 15) / 16, sdpa_anyd_tv(), (g.Dv + 31) / 32, [&](auto ds, auto tv) {
		hipLaunchKernelGGL(HIP_KERNEL_NAME(sdpa_fwd_anyd_f16_kernel<decltype(ds)::value, decltype(tv)::value>), grid, dim3(256), 0, stream, g, qp, kp, vp, mp, op, lse); });
	HIP_ENFORCE(hipGetLastError());
}
