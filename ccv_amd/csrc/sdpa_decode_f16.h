// SCALED_DOT_PRODUCT_ATTENTION forward on CCV_16F tensors for FEW QUERY ROWS against a long key / value cache: the decode step of a language model (included by
// cmd_attention.cpp, inside its namespace, behind sdpa_geom_t, visible_keys and sdpa_anyd_f16.h).  The other forward kernels give a workgroup per (128 query rows,
// QUERY head, batch) and walk every key in it: with R = 1 that is B Hq workgroups of which one wave in four has a row, 31 of its 32 MFMA rows padding, and the
// query heads of one key head each read that head's K and V again.  Here
//   packing     the M = R ratio (<= 32) rows of ONE KEY HEAD are one MFMA row tile: packed row p = query row x = p / ratio of query head hk ratio + p % ratio.
//               Rows p >= M are zeros in the q registers and never stored.  Every K / V byte of a key head leaves HBM once per command.
//   split       grid (splits, Hk, B): a split owns a contiguous range of 32-key blocks, inside the workgroup wave w owns the blocks w, w + 4, ... of the range;
//               each wave keeps its own running maximum, sum and O^T accumulator -- NO workgroup barrier in the key loop.
// Per block and wave, the operand layouts of sdpa_anyd_f16.h:
//   S^T [32 keys x 32 rows] = K Q^T    A = the lane's 16-byte fragment of key row l & 31, halves 16 s + 8 (l >> 5) .. + 7, loaded STRAIGHT from global memory (K never
//                                      touches LDS: nothing is shared between waves, and the fragment of a row IS the operand); B = the lane's q chunk, in
//                                      registers for the whole kernel (read again per block beside eight output tiles).  A q chunk past D is zeros in the
//                                      registers; K reads a chunk past D and a key past C from inside the tensor (below), never padded memory.
//   O^T [Dv x 32 rows] += V^T P^T      V lies in a WAVE-PRIVATE LDS tile as it lies in memory ([key][Dv], pitch sdpa_anyd_vpitch), one 16-byte store per chunk, and is
//                                      read back transposed (isa.h tr_read4) as A; B = the probabilities in the registers they were computed in.  Between the wave's
//                                      stores and its transposed reads: a wave barrier and NNC_WAIT_LGKM0, nothing wider.
// Pipeline: the K fragments and V chunks of the wave's NEXT block are issued right behind the current block's first product, INTO the registers it has just read,
// in front of the softmax and the second product, and waited for at the top of the next block (DS + 2 TV 16-byte registers per lane beside DS of q and 16 TV of
// O^T).  Issued in front of the first product they need a second set of DS registers: 100 - 290 bytes of scratch in the eight-tile instances.
// Softmax in fp32 in the base-2 domain as in the other forward kernels; the lane's visible-key count and mask row are those of ITS packed row (b, h, x).  Blocks past
// the last row's visible keys (visible_keys() does not fall with x) are in no wave's range.
// End of a workgroup: the waves' (m, l, O^T) meet in LDS in wave order (the V tiles' memory, fp32 [16 TV][64 lanes] + m, l: 4096 TV + 512 bytes <= 4 tiles), wave 0
// merges.  splits == 1: it normalises and writes the half output and the log-sum-exp -- one launch.  Otherwise it writes the fp32 partial (m, l, -, -, O[Dv]) of
// (b, hk, split, p) and sdpa_decode_fold_kernel folds the partials in split order -- no atomics: the same tensors give the same bits on every run.  A split or wave
// that saw no key (m = -inf, l = 0) contributes nothing; a row that sees no key at all gives 0 and -inf.
// LDS: four tiles of 32 x sdpa_anyd_vpitch<TV> halves: 73,728 bytes at Dv = 256.  Instances: DS in {2, 4, 8, 12, 16} x TV in {1, 2, 4, 8}, the steps and tiles past
// D / Dv skipped wave-uniformly.
#pragma once

// a fence for the machine scheduler between the phases of a block: loads, products and the per-tile loops stay in program order (it does not lower the register
// count: the allocation of the accumulators decides that)
#ifdef NNC_HIP_EMULATOR
#define SDPA_DECODE_SCHED() ((void)0)
#else
#define SDPA_DECODE_SCHED() __builtin_amdgcn_sched_barrier(0)
#endif
constexpr int SDPA_DECODE_ROWS = 32; // packed rows of one workgroup: one MFMA tile

template <int DS, int TV>
__global__ void __launch_bounds__(256) sdpa_decode_f16_kernel(const sdpa_geom_t g, const int M, const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, const half_t* __restrict__ mask, half_t* __restrict__ o, float* __restrict__ lse, float* __restrict__ partial)
{
	constexpr int VP = sdpa_anyd_vpitch<TV>();
	constexpr int VCH = 4 * TV, NV = 2 * TV; // 16-byte chunks per key row of the tile, per lane and block (32 VCH / 64)
	__shared__ __attribute__((aligned(16))) half_t Vs[4 * 32 * VP];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int li = lane & 31, lh = lane >> 5;
	const int split = blockIdx.x, splits = gridDim.x, hk = blockIdx.y, b = blockIdx.z;
	const bool row = li < M;
	const int x = row ? li / g.ratio : 0, h = hk * g.ratio + (row ? li % g.ratio : 0);
	const int ds_n = (g.D + 15) >> 4, tv_n = (g.Dv + 31) >> 5;
	const halfx8 zero8 = halfx8{ 0, 0, 0, 0, 0, 0, 0, 0 };
	// q: in registers for the whole kernel -- except beside eight output tiles, where 4 DS more registers do not fit without scratch: there the lane reads its
	// chunk again in every block (a few KB that stay in the CU's cache)
	constexpr bool QREG = TV < 8;
	constexpr int TG = TV < 8 ? 4 : 2; // output tiles whose transposed reads are in flight together
	const half_t* qrow = q + b * g.q_sb + (long)x * g.q_sr + h * g.q_sh + 8 * lh;
	halfx8 qf[QREG ? DS : 1];
#pragma unroll
	for (int s = 0; s < (QREG ? DS : 1); s++) {
		qf[s] = zero8;
		if (row && 16 * s + 8 * lh < g.D) qf[s] = *(const halfx8*)(qrow + 16 * s);
	}
	floatx16 acc[TV];
#pragma unroll
	for (int tv = 0; tv < TV; tv++)
#pragma unroll
		for (int r = 0; r < 16; r++) acc[tv][r] = 0.f;
	float m_run = -INFINITY, l_run = 0.f; // base-2 domain
	const int vis = row ? visible_keys(g, x) : 0;
	// the split's blocks [j0, j1) of the ceil(visible_keys(last row) / 32) that any row sees; this wave's: j0 + wave, + 4, ...
	const int nblk = (visible_keys(g, g.R - 1) + 31) >> 5, per = (nblk + splits - 1) / splits;
	const int j0 = split * per, j1 = j0 + per < nblk ? j0 + per : nblk;
	const float LOG2E = 1.4426950408889634f;
	const float c2 = g.scale * LOG2E;
	const half_t* const mrow = mask ? mask + b * g.m_sb + h * g.m_sh + (long)x * g.m_sr : 0;
	const half_t* const kbase = k + b * g.k_sb + hk * g.k_sh;
	const half_t* const vbase = v + b * g.v_sb + hk * g.v_sh;
	half_t* const Vw = Vs + wave * (32 * VP);
	halfx8 kf[DS], vr[NV];
	// the lane's K fragments (key y + li, one per step) and V chunks (chunk c = lane + 64 jj is key c / VCH, halves 8 (c % VCH) .. + 7) of the block at y.  No load is
	// predicated (a branch each, and no two in one clause) and none is followed by a select (a second register set): a key past C reads key C - 1 (a block has at
	// least one key), a chunk past D / Dv reads chunk 0 of the same row -- every address lies inside the tensor by construction -- and what they read never
	// shows: scores of keys past C are set to -inf below and their probabilities are 0, the q registers of a chunk past D are zeros, output columns past Dv are
	// not stored
	const int c_last = g.C - 1;
	const int vd = ((lane % VCH) << 3) < g.Dv ? (lane % VCH) << 3 : 0; // (VCH divides 64: the lane's columns are the same in every chunk)
#define SDPA_DECODE_FETCH(y) do { \
		const int yk = (y) + li < c_last ? (y) + li : c_last; \
		const half_t* const krow = kbase + (long)yk * g.k_sc + 8 * lh; \
		_Pragma("unroll") for (int s = 0; s < DS; s++) \
			if (s < ds_n) kf[s] = *(const halfx8*)(krow + (16 * s + 8 * lh < g.D ? 16 * s : -8 * lh)); \
		_Pragma("unroll") for (int jj = 0; jj < NV; jj++) { \
			const int j = (lane + 64 * jj) / VCH, yv = (y) + j < c_last ? (y) + j : c_last; \
			vr[jj] = *(const halfx8*)(vbase + (long)yv * g.v_sc + vd); \
		} } while (0)
#pragma unroll
	for (int s = 0; s < DS; s++) kf[s] = zero8;
	if (j0 + wave < j1) SDPA_DECODE_FETCH(32 * (j0 + wave));
	for (int jb = j0 + wave; jb < j1; jb += 4) {
		const int y0 = 32 * jb;
		__builtin_amdgcn_wave_barrier(); // every lane is done with the transposed reads of the block before
#pragma unroll
		for (int jj = 0; jj < NV; jj++) {
			const int c = lane + 64 * jj, j = c / VCH, d = (c - j * VCH) << 3;
			*(halfx8*)(Vw + j * VP + d) = vr[jj]; // as it lies: one 16-byte store per chunk
		}
		SDPA_DECODE_SCHED();
		int q0 = 0;
		if (!QREG) NNC_PIN_V(q0); // (an offset hipcc cannot see through, or it hoists the loads out of the loop: the registers again)
		floatx16 s;
#pragma unroll
		for (int r = 0; r < 16; r++) s[r] = 0.f;
#pragma unroll
		for (int i = 0; i < DS; i++)
			if (i < ds_n) {
				if (QREG) s = nnc_mfma_f16(kf[i], qf[i], s);
				else s = nnc_mfma_f16(kf[i], row && 16 * i + 8 * lh < g.D ? *(const halfx8*)(qrow + q0 + 16 * i) : zero8, s);
			}
		SDPA_DECODE_SCHED();
		if (jb + 4 < j1) SDPA_DECODE_FETCH(y0 + 128); // into the registers the products above have just read: in flight behind the softmax and the second product
		SDPA_DECODE_SCHED();
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
		for (int tv = 0; tv < TV; tv++) {
			if (tv < tv_n)
#pragma unroll
				for (int r = 0; r < 16; r++) acc[tv][r] *= alpha;
			SDPA_DECODE_SCHED(); // (the tiles in program order)
		}
		NNC_WAIT_LGKM0(); // the wave's own tile stores, nobody else's
		__builtin_amdgcn_wave_barrier();
		SDPA_DECODE_SCHED();
#pragma unroll
		for (int tt = 0; tt < 2; tt++) {
			const halfx8 pf = halfx8{ (half_t)s[8 * tt], (half_t)s[8 * tt + 1], (half_t)s[8 * tt + 2], (half_t)s[8 * tt + 3], (half_t)s[8 * tt + 4], (half_t)s[8 * tt + 5], (half_t)s[8 * tt + 6], (half_t)s[8 * tt + 7] }; // (not sdpa_half8: it moves the registers of one instance)
			const half_t* const blk = Vw + (16 * tt + 4 * lh) * VP + 16 * (li >> 4);
#pragma unroll
			for (int t0 = 0; t0 < TV; t0 += TG) { // TG output tiles per wait: the transpose reads are asm, hipcc does not count them
				if (t0 >= tv_n) break;
				halfx4 lo[TG], hi[TG];
#pragma unroll
				for (int u = 0; u < TG; u++)
					if (t0 + u < TV) { lo[u] = tr_read4(blk + 32 * (t0 + u), VP, li & 15); hi[u] = tr_read4(blk + 32 * (t0 + u) + 8 * VP, VP, li & 15); }
				NNC_WAIT_LGKM0();
#pragma unroll
				for (int u = 0; u < TG; u++)
					if (t0 + u < TV) { NNC_PIN_VEC(lo[u]); NNC_PIN_VEC(hi[u]); }
#pragma unroll
				for (int u = 0; u < TG; u++)
					if (t0 + u < TV) {
						if (t0 + u < tv_n) acc[t0 + u] = nnc_mfma_f16(halfx8{ lo[u][0], lo[u][1], lo[u][2], lo[u][3], hi[u][0], hi[u][1], hi[u][2], hi[u][3] }, pf, acc[t0 + u]);
					}
			}
		}
	}
#undef SDPA_DECODE_FETCH
	// the four waves' states meet in wave order: wave w lays (m, l, O^T) down lane by lane, wave 0 takes it up into its own
	float* const Os = (float*)Vs; // [16 TV][64]
	float* const Ms = Os + 16 * TV * 64; // [2][64]
#pragma unroll 1
	for (int w = 1; w < 4; w++) {
		__syncthreads(); // the tiles are free (w = 1) / wave 0 has taken wave w - 1's state up
		if (wave == w) {
			Ms[lane] = m_run; Ms[64 + lane] = l_run;
#pragma unroll
			for (int tv = 0; tv < TV; tv++)
#pragma unroll
				for (int r = 0; r < 16; r++) Os[(16 * tv + r) * 64 + lane] = acc[tv][r];
		}
		__syncthreads();
		if (wave == 0) {
			const float m_w = Ms[lane], l_w = Ms[64 + lane];
			const float m_new = fmaxf(m_run, m_w);
			const float m_sub = m_new == -INFINITY ? 0.f : m_new;
			const float a0 = nnc_fast_exp2(m_run - m_sub), aw = nnc_fast_exp2(m_w - m_sub);
			l_run = l_run * a0 + l_w * aw;
			m_run = m_new;
#pragma unroll
			for (int tv = 0; tv < TV; tv++) {
#pragma unroll
				for (int r = 0; r < 16; r++) acc[tv][r] = acc[tv][r] * a0 + Os[(16 * tv + r) * 64 + lane] * aw;
				SDPA_DECODE_SCHED(); // (the tiles in program order)
			}
		}
	}
	if (wave != 0 || !row) return;
	if (partial) { // (m, l, -, -, O[Dv]) of (b, hk, split, p): registers 4 r4 .. 4 r4 + 3 are dv = 32 tv + 8 r4 + 4 lh + 0..3
		float* const prow = partial + ((((long)b * g.Hk + hk) * splits + split) * M + li) * (g.Dv + 4);
		if (lh == 0) { prow[0] = m_run; prow[1] = l_run; }
#pragma unroll
		for (int tv = 0; tv < TV; tv++)
#pragma unroll
			for (int r4 = 0; r4 < 4; r4++) {
				const int dv = 32 * tv + 8 * r4 + 4 * lh;
				if (dv < g.Dv) *(floatx4*)(prow + 4 + dv) = floatx4{ acc[tv][4 * r4], acc[tv][4 * r4 + 1], acc[tv][4 * r4 + 2], acc[tv][4 * r4 + 3] };
			}
		return;
	}
	const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
	half_t* const orow = o + b * g.o_sb + (long)x * g.o_sr + h * g.o_sh;
#pragma unroll
	for (int tv = 0; tv < TV; tv++)
#pragma unroll
		for (int r4 = 0; r4 < 4; r4++) {
			const int dv = 32 * tv + 8 * r4 + 4 * lh;
			if (dv < g.Dv) *(halfx4*)(orow + dv) = halfx4{ (half_t)(acc[tv][4 * r4] * inv), (half_t)(acc[tv][4 * r4 + 1] * inv), (half_t)(acc[tv][4 * r4 + 2] * inv), (half_t)(acc[tv][4 * r4 + 3] * inv) };
		}
	if (lse && lh == 0) lse[((long)b * g.Hq + h) * g.R + x] = l_run > 0.f ? (m_run + log2f(l_run)) * 0.6931471805599453f : -INFINITY;
}

// o, lse of packed row p of (b, hk) from the partials of its splits, in split order: m* = max m_s, O = sum 2^(m_s - m*) O_s / sum 2^(m_s - m*) l_s.  A thread per
// (row, four output columns).
__global__ void __launch_bounds__(256) sdpa_decode_fold_kernel(const sdpa_geom_t g, const int M, const int splits, const float* __restrict__ partial, half_t* __restrict__ o, float* __restrict__ lse)
{
	const int groups = g.Dv >> 2;
	const long i = blockIdx.x * 256l + threadIdx.x;
	if (i >= (long)g.B * g.Hk * M * groups) return;
	const int dg = (int)(i % groups);
	const long prow = i / groups;
	const int p = (int)(prow % M);
	const long bh = prow / M;
	const int hk = (int)(bh % g.Hk), b = (int)(bh / g.Hk);
	const int x = p / g.ratio, h = hk * g.ratio + p % g.ratio;
	const long ps = g.Dv + 4, ss = (long)M * ps; // floats per row, per split
	const float* const base = partial + (bh * splits * M + p) * ps;
	float m = -INFINITY;
	for (int s = 0; s < splits; s++) m = fmaxf(m, base[s * ss]);
	const float m_sub = m == -INFINITY ? 0.f : m;
	float l = 0.f;
	floatx4 acc = floatx4{ 0.f, 0.f, 0.f, 0.f };
	for (int s = 0; s < splits; s++) {
		const float a = nnc_fast_exp2(base[s * ss] - m_sub); // 0 for a split that saw no key
		l += a * base[s * ss + 1];
		const floatx4 os = *(const floatx4*)(base + s * ss + 4 + 4 * dg);
		acc[0] += a * os[0]; acc[1] += a * os[1]; acc[2] += a * os[2]; acc[3] += a * os[3];
	}
	const float inv = l > 0.f ? 1.f / l : 0.f;
	*(halfx4*)(o + b * g.o_sb + (long)x * g.o_sr + h * g.o_sh + 4 * dg) = halfx4{ (half_t)(acc[0] * inv), (half_t)(acc[1] * inv), (half_t)(acc[2] * inv), (half_t)(acc[3] * inv) };
	if (lse && dg == 0) lse[((long)b * g.Hq + h) * g.R + x] = l > 0.f ? (m + log2f(l)) * 0.6931471805599453f : -INFINITY;
}

// workgroups per CU the chosen split count aims at: measured (tools/attention_decode_bench.py) -- one a CU beats two and four at every C of
// the grouped-query rows (a workgroup holds a CU's registers nearly alone, and every split costs the fold a partial)
constexpr int SDPA_DECODE_WG_PER_CU = 1;

// D % 8 == 0, Dv % 8 == 0, 8 <= D, Dv <= 256, R ratio <= 32; 16-byte aligned q / k / v rows, 8-byte aligned o rows (the caller checks)
static int sdpa_decode_f16_run(const sdpa_geom_t& g, const half_t* const qp, const half_t* const kp, const half_t* const vp, const half_t* const mp, half_t* const op, float* const lse, ccv_nnc_stream_context_t* const ctx)
{
	const int M = g.R * g.ratio;
	const long nblk = (g.C + 31) / 32; // (the last row sees every key, causal or not: visible_keys(g, R - 1) == C)
	long splits = tune(TUNE_SDPA_DECODE_SPLITS);
	if (splits <= 0) { // enough workgroups for SDPA_DECODE_WG_PER_CU a CU, no split shorter than a block for each wave; 1 where B Hk alone fill the device
		const long heads = (long)g.B * g.Hk, cus = device_cu_count();
		splits = heads >= cus ? 1 : ((long)SDPA_DECODE_WG_PER_CU * cus + heads - 1) / heads;
		if (splits > nblk / 4) splits = nblk / 4;
	}
	if (splits < 1) splits = 1;
	if (splits > 65535) splits = 65535;
	float* partial = 0;
	if (splits > 1) {
		partial = (float*)workspace_of(ctx, sizeof(float) * (size_t)g.B * g.Hk * (size_t)splits * M * (g.Dv + 4));
		if (!partial) return CCV_NNC_EXEC_OOM;
	}
	hipStream_t stream = stream_of(ctx);
	const dim3 grid((unsigned)splits, g.Hk, g.B);
	note_kernel("sdpa_fwd_decode_f16");
	const double kv_bytes = 2.0 * g.B * g.Hk * (double)g.C * (g.D + g.Dv), qo_bytes = 2.0 * g.B * g.Hq * (double)g.R * (g.D + g.Dv);
	{
		ProfScope prof("sdpa_fwd_h_decode|nnc::sdpa_decode_f16_kernel", 2.0 * g.B * g.Hq * (double)g.R * g.C * (g.D + g.Dv), kv_bytes + qo_bytes, g.R, g.C, g.D, g.B * g.Hq, (int)splits, stream);
		sdpa_pick(sdpa_ints<2, 4, 8, 12, 16>(), (g.D + 15) / 16, sdpa_ints<1, 2, 4, 8>(), (g.Dv + 31) / 32, [&](auto ds, auto tv) {
			hipLaunchKernelGGL(HIP_KERNEL_NAME(sdpa_decode_f16_kernel<decltype(ds)::value, decltype(tv)::value>), grid, dim3(256), 0, stream, g, M, qp, kp, vp, mp, op, lse, partial); });
		HIP_ENFORCE(hipGetLastError());
	}
	if (splits > 1) {
		const long threads = (long)g.B * g.Hk * M * (g.Dv / 4);
		ProfScope prof("sdpa_fwd_h_decode_fold|nnc::sdpa_decode_fold_kernel", 0, 4.0 * g.B * g.Hk * (double)splits * M * (g.Dv + 4), M, g.Dv, (int)splits, g.B * g.Hk, 1, stream);
		hipLaunchKernelGGL(sdpa_decode_fold_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, g, M, (int)splits, (const float*)partial, op, lse);
		HIP_ENFORCE(hipGetLastError());
	}
	return CCV_NNC_EXEC_SUCCESS;
}
