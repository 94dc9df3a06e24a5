// SCALED_DOT_PRODUCT_ATTENTION forward on CCV_16F tensors for 33 .. 256 PACKED ROWS per key head against a long key / value cache: speculative-decoding verification,
// multi-query models with a few rows, the tail of a chunked prefill (included by cmd_attention.cpp, inside its namespace, behind sdpa_decode_f16.h, whose packing, partial
// layout, fold kernel and split key it shares).  sdpa_decode_f16_kernel stops at ONE MFMA row tile; a row more and the command went to the kernels that give a workgroup
// per (128 query rows, QUERY head, batch), walk every key in it and read a key head's K and V once per query head that shares it.  Here
//   packing     as in sdpa_decode_f16.h: packed row p = query row x = p / ratio of query head hk ratio + p % ratio, M = R ratio rows per key head.  Rows p >= M are zeros
//               in the q registers and never stored.
//   split       grid (splits x groups, Hk, B): a workgroup is T waves (T = 2 while M <= 64, else 4), wave w owns the 32-row tile w of its group of 32 T packed rows,
//               M > 128 takes ceil(M / 128) groups.  EVERY wave of a workgroup walks the SAME 32-key blocks of its split: the key axis is split by the grid alone, so
//               nothing is merged inside the workgroup -- each wave keeps the running maximum, sum and O^T accumulator of its own rows from the first block to the last.
//   tiles       a 32-key block of K ([32][16 DS + 8 halves]: sdpa_anyd_f16.h's pitch, 4 (mod 8) dwords -- the 16-byte fragment reads of a 16-lane group do not collide)
//               and of V (as it lies, [32][sdpa_anyd_vpitch<TV>]) goes global -> registers -> LDS ONCE per workgroup, the 64 T threads sharing the 16-byte chunks
//               (chunk c = t + 64 T jj: key c / chunks-per-row); every wave reads its K fragments back as the A operand of S^T = K Q^T (ds_read_b128) and V transposed
//               (isa.h tr_read4) as the A operand of O^T += V^T P^T.  A K / V byte leaves HBM once per GROUP, not once per query head.
//   pipeline    TWO LDS buffers, ONE __syncthreads() per block: behind the barrier that publishes block j the loads of block j + 1 are issued, in front of the products
//               of block j, and stored into the OTHER buffer behind them.  (The barrier at the top of block j + 1 publishes them; the buffer they overwrite was last read
//               in block j - 1, in front of the barrier at the top of block j.)
//   barriers    every wave of a workgroup reaches every barrier the same number of times: the trip count [j0, j1) is a function of (split, group) alone -- the blocks the
//               group's LAST row sees, cut into `splits` ranges -- and no wave leaves before the loop ends.  A wave whose tile is empty (p >= M) or whose rows see nothing of
//               a block (the causal triangle) skips the products, never the loads, the stores or the barrier.
// Loads are never predicated into padded memory (sdpa_decode_f16.h's rule): a key past C reads key C - 1, a chunk past D / Dv reads chunk 0 of the same row; scores of keys
// past the lane's visible keys are -inf, the q registers of a chunk past D are zeros, output columns past Dv are not stored.  Threads past the last chunk of a tile (DS = 2
// or TV = 1 under 256 threads: whole waves) neither load nor store.
// Softmax in fp32 in the base-2 domain per lane row, with the lane's own visible-key count and mask row.  q stays in registers, except beside eight output tiles
// (sdpa_decode_f16.h's QREG exception).  splits == 1: each wave normalises and writes the half output and the log-sum-exp of its rows.  Otherwise it writes the fp32
// partial (m, l, -, -, O[Dv]) of (b, hk, split, p) and sdpa_decode_fold_kernel folds the partials in split order -- no atomics anywhere.  A split that saw no key writes
// (-inf, 0, 0...), which the fold ignores; a row that sees no key gives 0 and -inf.
// LDS: 2 x 32 x (16 DS + 8 + sdpa_anyd_vpitch<TV>) halves -- 70,656 bytes at D = Dv = 256 (DS 16, TV 8), 9,216 at DS 2, TV 1.
// Instances: DS in {2, 4, 8, 12, 16} x TV in {1, 2, 4, 8} x T in {2, 4}, the steps and tiles past D / Dv skipped wave-uniformly.
#pragma once

constexpr int SDPA_DECODE_TILES_MAX = 8; // row tiles per key head the route may ask for (key SDPA_DECODE_TILES)

template <int DS, int TV, int T>
__global__ void __launch_bounds__(64 * T) sdpa_decode_tiles_f16_kernel(const sdpa_geom_t g, const int M, const int groups, const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, const half_t* __restrict__ mask, half_t* __restrict__ o, float* __restrict__ lse, float* __restrict__ partial)
{
	constexpr int NT = 64 * T, KP = 16 * DS + 8, VP = sdpa_anyd_vpitch<TV>();
	constexpr int KCH = 2 * DS, VCH = 4 * TV; // 16-byte chunks per key row of the tiles
	constexpr int NK = (32 * KCH + NT - 1) / NT, NV = (32 * VCH + NT - 1) / NT; // chunks per thread and block
	constexpr int TILE = 32 * (KP + VP); // halves of one buffer: the K tile, the V tile behind it
	__shared__ __attribute__((aligned(16))) half_t Ls[2 * TILE];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const int li = lane & 31, lh = lane >> 5;
	const int grp = blockIdx.x % groups, split = blockIdx.x / groups, splits = gridDim.x / groups, hk = blockIdx.y, b = blockIdx.z;
	const int p0 = (grp * T + wave) * 32, p = p0 + li; // the wave's tile, the lane's packed row
	const bool row = p < M;
	const int x = row ? p / g.ratio : 0, h = hk * g.ratio + (row ? p % g.ratio : 0);
	const int ds_n = (g.D + 15) >> 4, tv_n = (g.Dv + 31) >> 5;
	const halfx8 zero8 = halfx8{ 0, 0, 0, 0, 0, 0, 0, 0 };
	constexpr bool QREG = TV < 8; // (sdpa_decode_f16.h: beside eight output tiles the lane reads its q chunk again in every block)
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
	// keys the group's / the wave's last row sees (visible_keys() does not fall with x, x does not fall with p); an empty tile sees none
	const int pg = (grp + 1) * 32 * T < M ? (grp + 1) * 32 * T : M, pw = p0 + 32 < M ? p0 + 32 : M;
	const int vis_grp = visible_keys(g, (pg - 1) / g.ratio), vis_wave = p0 < M ? visible_keys(g, (pw - 1) / g.ratio) : 0;
	// the split's blocks [j0, j1) of the group's ceil(vis_grp / 32): the same for every wave and lane of the workgroup
	const int nblk = (vis_grp + 31) >> 5, per = (nblk + splits - 1) / splits;
	const int j0 = split * per, j1 = j0 + per < nblk ? j0 + per : nblk;
	const float LOG2E = 1.4426950408889634f;
	const float c2 = g.scale * LOG2E;
	const half_t* const mrow = mask ? mask + b * g.m_sb + h * g.m_sh + (long)x * g.m_sr : 0;
	const half_t* const kbase = k + b * g.k_sb + hk * g.k_sh;
	const half_t* const vbase = v + b * g.v_sb + hk * g.v_sh;
	const int c_last = g.C - 1;
	const int vj = t / VCH, vd = ((t % VCH) << 3) < g.Dv ? (t % VCH) << 3 : 0; // (VCH divides 64 T: the thread's V columns are the same in every chunk)
	halfx8 kr[NK], vr[NV];
	// the thread's chunks of the key block at y into kr / vr; every address lies inside the tensor by construction (above)
#define SDPA_TILES_FETCH(y) do { \
		_Pragma("unroll") for (int jj = 0; jj < NK; jj++) { \
			const int c = t + NT * jj, j = c / KCH, d = (c - j * KCH) << 3; \
			const int yk = (y) + j < c_last ? (y) + j : c_last; \
			if (c < 32 * KCH) kr[jj] = *(const halfx8*)(kbase + (long)yk * g.k_sc + (d < g.D ? d : 0)); \
		} \
		_Pragma("unroll") for (int jj = 0; jj < NV; jj++) { \
			const int j = vj + (NT / VCH) * jj, yv = (y) + j < c_last ? (y) + j : c_last; \
			if (t + NT * jj < 32 * VCH) vr[jj] = *(const halfx8*)(vbase + (long)yv * g.v_sc + vd); \
		} } while (0)
	// ... and from the registers into the buffer at `buf`: K rows of KP halves, V as it lies behind them
#define SDPA_TILES_STORE(buf) do { \
		_Pragma("unroll") for (int jj = 0; jj < NK; jj++) { \
			const int c = t + NT * jj, j = c / KCH, d = (c - j * KCH) << 3; \
			if (c < 32 * KCH) *(halfx8*)((buf) + j * KP + d) = kr[jj]; \
		} \
		_Pragma("unroll") for (int jj = 0; jj < NV; jj++) \
			if (t + NT * jj < 32 * VCH) *(halfx8*)((buf) + 32 * KP + (vj + (NT / VCH) * jj) * VP + ((t % VCH) << 3)) = vr[jj]; \
		} while (0)
	if (j0 < j1) {
		SDPA_TILES_FETCH(32 * j0);
		SDPA_TILES_STORE(Ls);
	}
	int cur = 0;
	for (int jb = j0; jb < j1; jb++) { // (uniform in the workgroup: one barrier per trip, for every wave)
		const int y0 = 32 * jb;
		const half_t* const Ks = Ls + cur * TILE;
		const half_t* const Vs = Ks + 32 * KP;
		__syncthreads(); // this block's tiles are published; every wave is done with the other buffer (read in the block before)
		const bool more = jb + 1 < j1;
		if (more) SDPA_TILES_FETCH(y0 + 32); // in flight behind the products below
		SDPA_DECODE_SCHED();
		if (y0 < vis_wave) { // (wave-uniform; the loads, the stores and the barrier are outside)
			int q0 = 0;
			if (!QREG) NNC_PIN_V(q0); // (an offset hipcc cannot see through, or it hoists the loads out of the loop: the registers again)
			floatx16 s;
#pragma unroll
			for (int r = 0; r < 16; r++) s[r] = 0.f;
#pragma unroll
			for (int i = 0; i < DS; i++)
				if (i < ds_n) {
					const halfx8 kf = *(const halfx8*)(Ks + li * KP + 16 * i + 8 * lh);
					if (QREG) s = nnc_mfma_f16(kf, qf[i], s);
					else s = nnc_mfma_f16(kf, row && 16 * i + 8 * lh < g.D ? *(const halfx8*)(qrow + q0 + 16 * i) : zero8, s);
				}
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
#pragma unroll
			for (int tt = 0; tt < 2; tt++) {
				const halfx8 pf = halfx8{ (half_t)s[8 * tt], (half_t)s[8 * tt + 1], (half_t)s[8 * tt + 2], (half_t)s[8 * tt + 3], (half_t)s[8 * tt + 4], (half_t)s[8 * tt + 5], (half_t)s[8 * tt + 6], (half_t)s[8 * tt + 7] };
				const half_t* const blk = Vs + (16 * tt + 4 * lh) * VP + 16 * (li >> 4);
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
		SDPA_DECODE_SCHED();
		if (more) SDPA_TILES_STORE(Ls + (cur ^ 1) * TILE); // the other buffer: nobody reads it before the next barrier
		cur ^= 1;
	}
#undef SDPA_TILES_FETCH
#undef SDPA_TILES_STORE
	if (!row) return; // (behind the last barrier)
	if (partial) { // (m, l, -, -, O[Dv]) of (b, hk, split, p): registers 4 r4 .. 4 r4 + 3 are dv = 32 tv + 8 r4 + 4 lh + 0..3
		float* const prow = partial + ((((long)b * g.Hk + hk) * splits + split) * M + p) * (g.Dv + 4);
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

// 32-key blocks a split is at least long, where the launch chooses the splits: measured (tools/attention_decode_bench.py --min-blocks)
constexpr int SDPA_DECODE_TILES_MIN_BLOCKS = 4;

// D % 8 == 0, Dv % 8 == 0, 8 <= D, Dv <= 256, 32 < R ratio <= 32 SDPA_DECODE_TILES_MAX; 16-byte aligned q / k / v rows, 8-byte aligned o rows (the caller checks)
static int sdpa_decode_tiles_f16_run(const sdpa_geom_t& g, const half_t* const qp, const half_t* const kp, const half_t* const vp, const half_t* const mp, half_t* const op, float* const lse, ccv_nnc_stream_context_t* const ctx)
{
	const int M = g.R * g.ratio, T = M <= 64 ? 2 : 4, groups = (M + 32 * T - 1) / (32 * T);
	const long nblk = (g.C + 31) / 32; // (the last row sees every key, causal or not)
	long splits = tune(TUNE_SDPA_DECODE_SPLITS);
	if (splits <= 0) { // about SDPA_DECODE_WG_PER_CU workgroups a CU, no split shorter than SDPA_DECODE_TILES_MIN_BLOCKS blocks; 1 where B Hk groups alone fill the device
		const long wgs = (long)g.B * g.Hk * groups, cus = device_cu_count();
		splits = wgs >= cus ? 1 : ((long)SDPA_DECODE_WG_PER_CU * cus + wgs - 1) / wgs;
		if (splits > nblk / SDPA_DECODE_TILES_MIN_BLOCKS) splits = nblk / SDPA_DECODE_TILES_MIN_BLOCKS;
	}
	if (splits < 1) splits = 1;
	if (splits > 65535) splits = 65535;
	float* partial = 0;
	if (splits > 1) {
		partial = (float*)workspace_of(ctx, sizeof(float) * (size_t)g.B * g.Hk * (size_t)splits * M * (g.Dv + 4));
		if (!partial) return CCV_NNC_EXEC_OOM;
	}
	hipStream_t stream = stream_of(ctx);
	const dim3 grid((unsigned)(splits * groups), g.Hk, g.B);
	note_kernel("sdpa_fwd_decode_tiles_f16");
	const double kv_bytes = 2.0 * g.B * g.Hk * (double)groups * g.C * (g.D + g.Dv), qo_bytes = 2.0 * g.B * g.Hq * (double)g.R * (g.D + g.Dv);
	{
		ProfScope prof("sdpa_fwd_h_decode_tiles|nnc::sdpa_decode_tiles_f16_kernel", 2.0 * g.B * g.Hq * (double)g.R * g.C * (g.D + g.Dv), kv_bytes + qo_bytes, g.R, g.C, g.D, g.B * g.Hq, (int)splits, stream);
		sdpa_pick(sdpa_ints<2, 4>(), T, [&](auto tw) {
			sdpa_pick(sdpa_ints<2, 4, 8, 12, 16>(), (g.D + 15) / 16, sdpa_ints<1, 2, 4, 8>(), (g.Dv + 31) / 32, [&](auto ds, auto tv) {
				hipLaunchKernelGGL(HIP_KERNEL_NAME(sdpa_decode_tiles_f16_kernel<decltype(ds)::value, decltype(tv)::value, decltype(tw)::value>), grid, dim3(64 * decltype(tw)::value), 0, stream, g, M, groups, qp, kp, vp, mp, op, lse, partial); }); });
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
