// UPSAMPLE (nearest / bilinear, align_corners or not), forward and backward, NCHW and NHWC, on gfx950 -- the
// resolution changes of the diffusion UNets.  Oracle: lib/nnc/cmd/upsample/ccv_nnc_upsample_cpu_ref.c
//   nearest  :16-208   source index = min((int)((xd + 0.5) r), A - 1), or (int)(xd r + 0.5) with align_corners; backward adds every output
//                      gradient into its source
//   bilinear :214-526  per axis (_ccv_nnc_init_bi_coeffs :218-243): xs = (i + 0.5) s - 0.5 (or i s), taps si0 = (int)xs, si1 = min((int)(xs + 1), A - 1),
//                      weights sc1 = xs - si0, sc0 = 1 - sc1 (xs < 0 gives a NEGATIVE sc1: kept); backward scatters g with the same weights
// Every coefficient is recomputed per thread with the reference's exact mixed float / double expression, so the taps agree bit for bit.
// Backward is a GATHER: one thread per input-gradient element walks the (few) outputs that reference it in (yd, xd, tap) order -- the order
// the reference's sequential scatter adds them -- so sums are bit-identical without atomics.  HBM-bound, 4 bytes per lane.
#include "upsample_ops.h" // UpGeom, nearest_src, bi_coeff, upsample_geometry; the half kernels and their plan

using namespace nnc;

namespace {

__device__ __forceinline__ void split4(size_t idx, const int d1, const int d2, const int d3, int& i0, int& i1, int& i2, int& i3)
{
	i3 = (int)(idx % d3); idx /= d3;
	i2 = (int)(idx % d2); idx /= d2;
	i1 = (int)(idx % d1); idx /= d1;
	i0 = (int)idx;
}

template <int TYPE>
__global__ void __launch_bounds__(256) upsample_forw_kernel(const UpGeom g, const float* a, float* b, const size_t total)
{
#pragma clang fp contract(off) // the reference rounds every product and sum separately; hipcc would fuse them into FMAs (last-ulp differences)
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
		int n, c, yd, xd;
		if (g.nchw) split4(idx, g.C, g.BH, g.BW, n, c, yd, xd); else split4(idx, g.BH, g.BW, g.C, n, yd, xd, c);
		const float* const ap = a + (long)n * g.an + (long)c * g.ac;
		float v;
		if (TYPE == UPSAMPLE_NEAREST) v = ap[(long)nearest_src(yd, g.rh, g.AH, g.align) * g.ah + (long)nearest_src(xd, g.rw, g.AW, g.align) * g.aw];
		else {
			const Bi y = bi_coeff(yd, g.rh, g.AH, g.align), x = bi_coeff(xd, g.rw, g.AW, g.align);
			const float a00 = ap[(long)y.si0 * g.ah + (long)x.si0 * g.aw], a01 = ap[(long)y.si0 * g.ah + (long)x.si1 * g.aw];
			const float a10 = ap[(long)y.si1 * g.ah + (long)x.si0 * g.aw], a11 = ap[(long)y.si1 * g.ah + (long)x.si1 * g.aw];
			// the two layouts of the reference round differently: NCHW multiplies tap * sc_x * sc_y (:304-305), NHWC pre-multiplies the weights (:344-355)
			if (g.nchw) v = a00 * x.sc0 * y.sc0 + a01 * x.sc1 * y.sc0 + a10 * x.sc0 * y.sc1 + a11 * x.sc1 * y.sc1;
			else v = a00 * (x.sc0 * y.sc0) + a01 * (x.sc1 * y.sc0) + a10 * (x.sc0 * y.sc1) + a11 * (x.sc1 * y.sc1);
		}
		b[(long)n * g.bn + (long)c * g.bc + (long)yd * g.bh + (long)xd * g.bw] = v;
	}
}

// candidate outputs that can reference source index s along an axis of A sources / B outputs
__device__ __forceinline__ void window(const int s, const float r, const int B, int& lo, int& hi)
{
	const float inv = r > 0.f ? 1.f / r : 1.f;
	lo = (int)floorf(((float)s - 1.5f) * inv) - 2;
	hi = (int)ceilf(((float)s + 1.5f) * inv) + 2;
	if (lo < 0) lo = 0;
	if (hi > B - 1) hi = B - 1;
}
template <int TYPE>
__global__ void __launch_bounds__(256) upsample_back_kernel(const UpGeom g, const float* b, float* a, const size_t total)
{
#pragma clang fp contract(off)
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
		int n, c, ys, xs;
		if (g.nchw) split4(idx, g.C, g.AH, g.AW, n, c, ys, xs); else split4(idx, g.AH, g.AW, g.C, n, ys, xs, c);
		const float* const bp = b + (long)n * g.bn + (long)c * g.bc;
		int ylo, yhi, xlo, xhi;
		window(ys, g.rh, g.BH, ylo, yhi);
		window(xs, g.rw, g.BW, xlo, xhi);
		float sum = 0.f;
		for (int yd = ylo; yd <= yhi; yd++) {
			if (TYPE == UPSAMPLE_NEAREST) {
				if (nearest_src(yd, g.rh, g.AH, g.align) != ys) continue;
				for (int xd = xlo; xd <= xhi; xd++)
					if (nearest_src(xd, g.rw, g.AW, g.align) == xs) sum += bp[(long)yd * g.bh + (long)xd * g.bw];
			} else {
				const Bi y = bi_coeff(yd, g.rh, g.AH, g.align);
				const bool y0 = y.si0 == ys, y1 = y.si1 == ys;
				if (!y0 && !y1) continue;
				for (int xd = xlo; xd <= xhi; xd++) {
					const Bi x = bi_coeff(xd, g.rw, g.AW, g.align);
					const bool x0 = x.si0 == xs, x1 = x.si1 == xs;
					if (!x0 && !x1) continue;
					const float gv = bp[(long)yd * g.bh + (long)xd * g.bw];
					// tap order of the reference's scatter: (y0,x0) (y0,x1) (y1,x0) (y1,x1); NCHW: g * sc_y * sc_x (:425-428), NHWC: g * (sc_x * sc_y) (:470-481)
					if (g.nchw) {
						if (y0 && x0) sum += gv * y.sc0 * x.sc0;
						if (y0 && x1) sum += gv * y.sc0 * x.sc1;
						if (y1 && x0) sum += gv * y.sc1 * x.sc0;
						if (y1 && x1) sum += gv * y.sc1 * x.sc1;
					} else {
						if (y0 && x0) sum += gv * (x.sc0 * y.sc0);
						if (y0 && x1) sum += gv * (x.sc1 * y.sc0);
						if (y1 && x0) sum += gv * (x.sc0 * y.sc1);
						if (y1 && x1) sum += gv * (x.sc1 * y.sc1);
					}
				}
			}
		}
		a[(long)n * g.an + (long)c * g.ac + (long)ys * g.ah + (long)xs * g.aw] = sum;
	}
}

static bool dense_f32(const ccv_nnc_tensor_t* t) { return t && tensor_contiguous(t) && CCV_GET_DATA_TYPE(t->info.datatype) == CCV_32F; }

#define EXEC_ARGS const ccv_nnc_cmd_t cmd, const ccv_nnc_hint_t hint, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, ccv_nnc_stream_context_t* const stream_context

// the fp32 launch record: "upsample_forw|nnc::upsample_forw_kernel" / "upsample_back|nnc::upsample_back_kernel" (the half route through fp32 images files it too)
static int upsample_f32(const bool forward, const int type, const UpGeom& g, const float* in, float* out, const size_t total, ccv_nnc_stream_context_t* ctx)
{
	hipStream_t stream = stream_of(ctx);
	const double na = (double)g.N * g.C * g.AH * g.AW, nb = (double)g.N * g.C * g.BH * g.BW;
	note_kernel(forward ? "upsample_forw" : "upsample_back");
	ProfScope prof(forward ? "upsample_forw|nnc::upsample_forw_kernel" : "upsample_back|nnc::upsample_back_kernel", forward ? nb : na, sizeof(float) * (na + nb), g.N, g.C, g.BH, g.BW, 1, stream);
	const dim3 grid(grid_for(total, 256));
	if (forward && type == UPSAMPLE_NEAREST) hipLaunchKernelGGL(HIP_KERNEL_NAME(upsample_forw_kernel<UPSAMPLE_NEAREST>), grid, dim3(256), 0, stream, g, in, out, total);
	else if (forward) hipLaunchKernelGGL(HIP_KERNEL_NAME(upsample_forw_kernel<UPSAMPLE_BILINEAR>), grid, dim3(256), 0, stream, g, in, out, total);
	else if (type == UPSAMPLE_NEAREST) hipLaunchKernelGGL(HIP_KERNEL_NAME(upsample_back_kernel<UPSAMPLE_NEAREST>), grid, dim3(256), 0, stream, g, in, out, total);
	else hipLaunchKernelGGL(HIP_KERNEL_NAME(upsample_back_kernel<UPSAMPLE_BILINEAR>), grid, dim3(256), 0, stream, g, in, out, total);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}
// dense halves in a geometry upsample_ops.h takes: its kernels; everything else: the code below, as before
static bool upsample_half_route(const ccv_nnc_cmd_t cmd, const int flags, const ccv_nnc_tensor_t* small, const ccv_nnc_tensor_t* big, const bool forward, ccv_nnc_stream_context_t* ctx, int* ret)
{
	upsample_plan_t up;
	if (!small || !big || !upsample_half_plan(cmd, flags, small, big, &up)) return false;
	*ret = upsample_half_run(up, forward, ctx);
	return true;
}

static int _upsample_forw(EXEC_ARGS)
{
	int ret;
	if (input_size >= 1 && output_size >= 1 && upsample_half_route(cmd, flags, inputs[0], outputs[0], true, stream_context, &ret)) return ret;
	if (input_size < 1 || output_size < 1 || !dense_f32(inputs[0]) || !dense_f32(outputs[0])) return CCV_NNC_EXEC_INVALID;
	UpGeom g;
	if (!upsample_geometry(cmd, inputs[0], outputs[0], &g)) return CCV_NNC_EXEC_INVALID;
	const int type = cmd.info.upsample.type;
	if (g.rh > 1.f || g.rw > 1.f) return CCV_NNC_EXEC_INVALID; // enlargement only: the reference asserts the same in every variant (:44-45, :273-274)
	const size_t total = tensor_count(outputs[0]->info);
	if (total == 0) return CCV_NNC_EXEC_SUCCESS;
	if (type != UPSAMPLE_NEAREST && type != UPSAMPLE_BILINEAR) return CCV_NNC_EXEC_INVALID;
	return upsample_f32(true, type, g, (const float*)inputs[0]->data.f32, outputs[0]->data.f32, total, stream_context);
}
static int _upsample_back(EXEC_ARGS)
{ // inputs[0] = gradient at the resampled resolution -> outputs[0] = gradient at the source resolution
	int ret;
	if (input_size >= 1 && output_size >= 1 && upsample_half_route(cmd, flags, outputs[0], inputs[0], false, stream_context, &ret)) return ret;
	if (input_size < 1 || output_size < 1 || !dense_f32(inputs[0]) || !dense_f32(outputs[0])) return CCV_NNC_EXEC_INVALID;
	UpGeom g;
	if (!upsample_geometry(cmd, outputs[0], inputs[0], &g)) return CCV_NNC_EXEC_INVALID;
	const int type = cmd.info.upsample.type;
	if (g.rh > 1.f || g.rw > 1.f) return CCV_NNC_EXEC_INVALID;
	const size_t total = tensor_count(outputs[0]->info);
	if (total == 0) return CCV_NNC_EXEC_SUCCESS;
	if (type != UPSAMPLE_NEAREST && type != UPSAMPLE_BILINEAR) return CCV_NNC_EXEC_INVALID;
	return upsample_f32(false, type, g, (const float*)inputs[0]->data.f32, outputs[0]->data.f32, total, stream_context);
}

} // namespace

namespace nnc {
bool upsample_half_applies(const ccv_nnc_cmd_t cmd, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size)
{
	if (input_size < 1 || output_size < 1 || !inputs[0] || !outputs[0]) return false;
	const bool forward = cmd.cmd == CCV_NNC_UPSAMPLE_FORWARD;
	upsample_plan_t up;
	return upsample_half_plan(cmd, flags, forward ? inputs[0] : outputs[0], forward ? outputs[0] : inputs[0], &up);
}
} // namespace nnc

// Test hook: what the plan makes of a geometry (host arithmetic only, nothing is launched): 0 refused, else the vector width of the forward instance on
// 16-byte-aligned bases plus 16 times that of the backward one.  dims: N, C, AH, AW, BH, BW.
extern "C" int nnc_mi355x_debug_upsample_plan(const int nchw, const int dims[6], const int type, const int align_corners)
{
	nnc::upsample_plan_t up;
	if (!nnc::up_geom_fill(&up.g, nchw, dims[0], dims[1], dims[2], dims[3], dims[4], dims[5], align_corners) || !nnc::up_geom_native(up.g, type)) return 0;
	up.type = type; up.small = 0; up.big = 0;
	return nnc::up_vector_width(up, true) + 16 * nnc::up_vector_width(up, false);
}

#define NNC_REG(CMD, BACKEND, EXEC) \
	extern "C" void _register_command_##CMD##_backend_##BACKEND(ccv_nnc_cmd_backend_registry_t* const registry) \
	{ registry->tensor_formats = CCV_TENSOR_FORMAT_NCHW | CCV_TENSOR_FORMAT_NHWC; registry->tensor_datatypes = CCV_32F; registry->tensor_memory = CCV_TENSOR_GPU_MEMORY; registry->algorithms = 1; registry->exec = EXEC; NNC_HALF_STAGED(registry, EXEC); }

NNC_REG(CCV_NNC_UPSAMPLE_FORWARD, CCV_NNC_BACKEND_GPU_REF, _upsample_forw)
NNC_REG(CCV_NNC_UPSAMPLE_BACKWARD, CCV_NNC_BACKEND_GPU_REF, _upsample_back)
