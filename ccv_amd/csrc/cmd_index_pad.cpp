// INDEX_SELECT (embedding gather / scatter-add) and PAD (zero / replicate, backward = crop) on gfx950.
// Oracle semantics:
//   index select  lib/nnc/cmd/index/ccv_nnc_index_select_cpu_ref.c:13-98   b[i][:] = a[indices[i]][:] (int32 indices; fp32 indices
//                 interpolate between rows j and j+1); backward h = 0, then h[indices[i]][:] += g[i][:] in row order
//   pad           lib/nnc/cmd/pad/ccv_nnc_pad_cpu_ref.c:13-140              begin = cmd.info.size.dim[], end = cmd.info.pad.end[]
// Both are HBM-bound copies.  The scatter-add keeps the reference's summation order (rows visited in order per column) so that
// repeated indices give bit-identical sums.  Dense tensors (fp32 and half; index_ops.h, tunable INDEX_BACK_TILES): a wave per tile of destination rows
// and columns walks the sources that name its rows in order, accumulators in LDS, and writes the tile once.  Views and the key at 0: one thread per column walks
// the rows; columns are the parallel dimension.
// Dense CCV_16F tensors run on the kernels of index_ops.h as halves (tunable INDEX_PAD_HALF_NATIVE); everything else in half precision runs on fp32 images.
#include "index_ops.h" // index_lerp, the pad kernels; the half kernels, the tile scatter-add and their plans

using namespace nnc;

namespace {

// ---- index select -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) index_select_i32_kernel(const float* a, const int* idx, float* b, const int rows, const int cols, const long a_inc, const long b_inc)
{
	const size_t n = (size_t)rows * cols, stride = (size_t)gridDim.x * blockDim.x;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		const size_t r = i / cols, c = i - r * cols;
		b[r * b_inc + c] = a[(long)idx[r] * a_inc + c];
	}
}
__global__ void __launch_bounds__(256) index_select_f32_kernel(const float* a, const float* idx, float* b, const int rows, const int cols, const long a_inc, const long b_inc, const int a_rows)
{
	const size_t n = (size_t)rows * cols, stride = (size_t)gridDim.x * blockDim.x;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		const size_t r = i / cols, c = i - r * cols;
		const IdxLerp k = index_lerp_rows(idx[r], a_rows);
		b[r * b_inc + c] = index_lerp(a[(long)k.j0 * a_inc + c], a[(long)k.j1 * a_inc + c], k);
	}
}
__global__ void __launch_bounds__(256) index_scatter_add_kernel(const float* g, const int* idx, float* h, const int g_rows, const int cols, const long g_inc, const long h_inc)
{
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= cols) return;
	for (int i = 0; i < g_rows; i++) h[(long)idx[i] * h_inc + c] += g[(long)i * g_inc + c];
}
__global__ void __launch_bounds__(256) zero_rows_kernel(float* h, const int rows, const int cols, const long h_inc)
{
	const size_t n = (size_t)rows * cols, stride = (size_t)gridDim.x * blockDim.x;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		const size_t r = i / cols;
		h[r * h_inc + (i - r * cols)] = 0.f;
	}
}
static void rows_cols(const ccv_nnc_tensor_t* t, int* rows, int* cols, long* inc)
{ // index_select_cpu_ref.c:22-27: dim[0] rows, dim[1] columns (1-d: one column), row increment = stride[0] for views
	const int nd = tensor_nd(t->info.dim);
	*rows = t->info.dim[0];
	*cols = nd < 2 ? 1 : t->info.dim[1];
	*inc = *cols;
	if (CCV_IS_TENSOR_VIEW(t) && nd >= 2) *inc = ((const ccv_nnc_tensor_view_t*)t)->stride[0];
}
#define EXEC_ARGS const ccv_nnc_cmd_t cmd, const ccv_nnc_hint_t hint, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size, ccv_nnc_stream_context_t* const stream_context

static int _index_select_forw(EXEC_ARGS)
{
	if (input_size < 2 || output_size < 1 || !inputs[0] || !inputs[1] || !outputs[0]) return CCV_NNC_EXEC_INVALID;
	index_plan_t ip;
	if (index_half_plan(true, flags, inputs[0], outputs[0], inputs[1], &ip)) return index_gather_run(ip, stream_context); // dense halves: index_ops.h
	const ccv_nnc_tensor_t* a = inputs[0];
	const ccv_nnc_tensor_t* ind = inputs[1];
	ccv_nnc_tensor_t* b = outputs[0];
	const int dt = CCV_GET_DATA_TYPE(a->info.datatype), it = CCV_GET_DATA_TYPE(ind->info.datatype);
	if ((dt != CCV_32F && dt != CCV_32S) || tensor_nd(a->info.dim) > 2 || tensor_nd(b->info.dim) > 2 || !tensor_contiguous(ind)) return CCV_NNC_EXEC_INVALID;
	int a_rows, a_cols, b_rows, b_cols;
	long a_inc, b_inc;
	rows_cols(a, &a_rows, &a_cols, &a_inc);
	rows_cols(b, &b_rows, &b_cols, &b_inc);
	if (a_cols != b_cols || tensor_count(ind->info) != (size_t)b_rows) return CCV_NNC_EXEC_INVALID;
	if (b_rows == 0 || b_cols == 0) return CCV_NNC_EXEC_SUCCESS;
	const unsigned grid = grid_for((size_t)b_rows * b_cols, 256);
	// int32 payloads move as raw 32-bit words through the same kernel
	if (it == CCV_32S) hipLaunchKernelGGL(index_select_i32_kernel, dim3(grid), dim3(256), 0, stream_of(stream_context), (const float*)a->data.f32, (const int*)ind->data.i32, b->data.f32, b_rows, b_cols, a_inc, b_inc);
	else if (it == CCV_32F && dt == CCV_32F) hipLaunchKernelGGL(index_select_f32_kernel, dim3(grid), dim3(256), 0, stream_of(stream_context), (const float*)a->data.f32, (const float*)ind->data.f32, b->data.f32, b_rows, b_cols, a_inc, b_inc, a_rows);
	else return CCV_NNC_EXEC_INVALID;
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}
static int _index_select_back(EXEC_ARGS)
{ // (g, _, indices) -> h (, _)
	if (input_size < 3 || output_size < 1 || !inputs[0] || !inputs[2] || !outputs[0]) return CCV_NNC_EXEC_INVALID;
	const ccv_nnc_tensor_t* g = inputs[0];
	const ccv_nnc_tensor_t* ind = inputs[2];
	ccv_nnc_tensor_t* h = outputs[0];
	hipStream_t stream = stream_of(stream_context);
	index_plan_t ip;
	const bool half = index_half_plan(false, flags, h, g, ind, &ip);
	if (half || index_back_plan(flags, h, g, ind, &ip)) { // dense tensors: the tile kernel zeroes and sums in one launch (index_ops.h)
		if (output_size >= 2 && outputs[1] && tensor_contiguous(outputs[1])) HIP_ENFORCE(hipMemsetAsync(outputs[1]->data.u8, 0, tensor_count(outputs[1]->info) * datatype_size(CCV_GET_DATA_TYPE(outputs[1]->info.datatype)), stream));
		return half ? index_scatter_run<half_t>(ip, stream_context) : index_scatter_run<float>(ip, stream_context);
	}
	if (CCV_GET_DATA_TYPE(g->info.datatype) != CCV_32F || CCV_GET_DATA_TYPE(ind->info.datatype) != CCV_32S || tensor_nd(g->info.dim) > 2 || tensor_nd(h->info.dim) > 2 || !tensor_contiguous(ind)) return CCV_NNC_EXEC_INVALID;
	int g_rows, g_cols, h_rows, h_cols;
	long g_inc, h_inc;
	rows_cols(g, &g_rows, &g_cols, &g_inc);
	rows_cols(h, &h_rows, &h_cols, &h_inc);
	if (g_cols != h_cols || tensor_count(ind->info) != (size_t)g_rows) return CCV_NNC_EXEC_INVALID;
	if (h_rows > 0 && h_cols > 0) hipLaunchKernelGGL(zero_rows_kernel, dim3(grid_for((size_t)h_rows * h_cols, 256)), dim3(256), 0, stream, h->data.f32, h_rows, h_cols, h_inc);
	if (output_size >= 2 && outputs[1] && tensor_contiguous(outputs[1])) HIP_ENFORCE(hipMemsetAsync(outputs[1]->data.u8, 0, tensor_count(outputs[1]->info) * datatype_size(CCV_GET_DATA_TYPE(outputs[1]->info.datatype)), stream));
	if (g_rows > 0 && g_cols > 0) {
		note_kernel("index_scatter_add");
		ProfScope prof("index_select_back|nnc::index_scatter_add_kernel", (double)g_rows * g_cols, sizeof(float) * 3.0 * g_rows * g_cols, g_rows, g_cols, h_rows, 1, 1, stream);
		hipLaunchKernelGGL(index_scatter_add_kernel, dim3((g_cols + 255) / 256), dim3(256), 0, stream, (const float*)g->data.f32, (const int*)ind->data.i32, h->data.f32, g_rows, g_cols, g_inc, h_inc);
	}
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

// ---- pad ----------------------------------------------------------------------------------------------------------------------------
// the kernels and pad_args_fill: index_ops.h.  Dense halves run there; fp32 tensors and views below
static bool pad_half_route(const ccv_nnc_cmd_t cmd, const int flags, const ccv_nnc_tensor_t* small, const ccv_nnc_tensor_t* big, const bool forward, ccv_nnc_stream_context_t* ctx, int* ret)
{
	pad_plan_t pp;
	if (!small || !big || !pad_half_plan(cmd, flags, small, big, forward, &pp)) return false;
	*ret = pad_half_run(pp, forward, ctx);
	return true;
}
static int _pad_forw(EXEC_ARGS)
{
	int ret;
	if (input_size >= 1 && output_size >= 1 && pad_half_route(cmd, flags, inputs[0], outputs[0], true, stream_context, &ret)) return ret;
	if (input_size < 1 || output_size < 1 || !inputs[0] || !outputs[0] || CCV_GET_DATA_TYPE(inputs[0]->info.datatype) != CCV_32F) return CCV_NNC_EXEC_INVALID;
	pad_args_t m;
	if (!pad_args_fill(cmd, inputs[0], outputs[0], &m)) return CCV_NNC_EXEC_INVALID;
	const size_t n = (size_t)m.bd[0] * m.bd[1] * m.bd[2] * m.bd[3];
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	if (cmd.info.pad.type == PAD_ZERO) hipLaunchKernelGGL(HIP_KERNEL_NAME(pad_forw_kernel<float, PAD_ZERO>), dim3(grid_for(n, 256)), dim3(256), 0, stream_of(stream_context), (const float*)inputs[0]->data.f32, outputs[0]->data.f32, m, n);
	else if (cmd.info.pad.type == PAD_REPLICATE) hipLaunchKernelGGL(HIP_KERNEL_NAME(pad_forw_kernel<float, PAD_REPLICATE>), dim3(grid_for(n, 256)), dim3(256), 0, stream_of(stream_context), (const float*)inputs[0]->data.f32, outputs[0]->data.f32, m, n);
	else return CCV_NNC_EXEC_INVALID;
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}
static int _pad_back(EXEC_ARGS)
{ // g (padded shape) -> h (original shape): the crop (pad_cpu_ref.c:88-138)
	int ret;
	if (input_size >= 1 && output_size >= 1 && pad_half_route(cmd, flags, outputs[0], inputs[0], false, stream_context, &ret)) return ret;
	if (input_size < 1 || output_size < 1 || !inputs[0] || !outputs[0] || CCV_GET_DATA_TYPE(inputs[0]->info.datatype) != CCV_32F) return CCV_NNC_EXEC_INVALID;
	pad_args_t m;
	if (!pad_args_fill(cmd, outputs[0], inputs[0], &m)) return CCV_NNC_EXEC_INVALID;
	const size_t n = (size_t)m.ad[0] * m.ad[1] * m.ad[2] * m.ad[3];
	if (n == 0) return CCV_NNC_EXEC_SUCCESS;
	hipLaunchKernelGGL(HIP_KERNEL_NAME(pad_back_kernel<float>), dim3(grid_for(n, 256)), dim3(256), 0, stream_of(stream_context), (const float*)inputs[0]->data.f32, outputs[0]->data.f32, m, n);
	HIP_ENFORCE(hipGetLastError());
	return CCV_NNC_EXEC_SUCCESS;
}

} // namespace

namespace nnc {
bool index_pad_half_applies(const ccv_nnc_cmd_t cmd, const int flags, ccv_nnc_tensor_t* const* const inputs, const int input_size, ccv_nnc_tensor_t* const* const outputs, const int output_size)
{
	if (input_size < 1 || output_size < 1 || !inputs[0] || !outputs[0]) return false;
	index_plan_t ip;
	pad_plan_t pp;
	switch (cmd.cmd) {
		case CCV_NNC_INDEX_SELECT_FORWARD: return input_size >= 2 && index_half_plan(true, flags, inputs[0], outputs[0], inputs[1], &ip);
		case CCV_NNC_INDEX_SELECT_BACKWARD: return input_size >= 3 && index_half_plan(false, flags, outputs[0], inputs[0], inputs[2], &ip);
		case CCV_NNC_PAD_FORWARD: return pad_half_plan(cmd, flags, inputs[0], outputs[0], true, &pp);
		case CCV_NNC_PAD_BACKWARD: return pad_half_plan(cmd, flags, outputs[0], inputs[0], false, &pp);
	}
	return false;
}
} // namespace nnc

#define NNC_REG(CMD, BACKEND, DATATYPES, EXEC) \
	extern "C" void _register_command_##CMD##_backend_##BACKEND(ccv_nnc_cmd_backend_registry_t* const registry) \
	{ registry->tensor_formats = CCV_TENSOR_FORMAT_NCHW | CCV_TENSOR_FORMAT_NHWC | CCV_TENSOR_FORMAT_CHWN; registry->tensor_datatypes = (DATATYPES); registry->tensor_memory = CCV_TENSOR_GPU_MEMORY; registry->algorithms = 1; registry->exec = EXEC; NNC_HALF_STAGED(registry, EXEC); }

NNC_REG(CCV_NNC_INDEX_SELECT_FORWARD, CCV_NNC_BACKEND_GPU_REF, CCV_32F | CCV_32S, _index_select_forw)
NNC_REG(CCV_NNC_INDEX_SELECT_BACKWARD, CCV_NNC_BACKEND_GPU_REF, CCV_32F | CCV_32S, _index_select_back)
NNC_REG(CCV_NNC_PAD_FORWARD, CCV_NNC_BACKEND_GPU_REF, CCV_32F, _pad_forw)
NNC_REG(CCV_NNC_PAD_BACKWARD, CCV_NNC_BACKEND_GPU_REF, CCV_32F, _pad_back)
