// The two pieces of the palettized (CCV_QX) stream's layout that every kernel reading it needs (palette.cpp: the expansion; gemm_qx_f16.h: the contraction that
// decodes its weight operand on the way): the index bytes of a full block, and the bits of one group of eight elements.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace nnc {

// index bytes of a FULL block, as the host's quantiser lays them out (ccv_nnc_palettize.c: the `ui0` strides of each bit width)
__host__ __device__ __forceinline__ size_t index_bytes_per_block(const int qbits, const int nib)
{
	switch (qbits) {
		case 4: return (size_t)(nib / 2);
		case 5: return (size_t)(nib / 8) * 5;
		case 6: return (size_t)(nib / 4) * 3;
		case 7: return (size_t)(nib / 8) * 7;
		default: return (size_t)nib;
	}
}

// One group: up to eight elements starting at element 8 g of a block.  `idx` points at the group's first index byte, `valid` (1 .. 8) elements exist.
// Fast path (a full group whose eight bytes idx[0 .. 7] all lie inside the stream -- every group but the stream's last one or two): ONE 8-byte load (gfx950
// global loads need no alignment), a byte swap, and a constant shift + mask per element.  Otherwise byte by byte, and only the index bytes the group's
// elements touch are read (the stream of the tensor's last block ends with them).
template <int Q>
__device__ __forceinline__ unsigned long long group_bits(const unsigned char* const idx, const int valid, const bool whole)
{ // the group's Q bytes as one big-endian number in the TOP 8 Q bits of the result: element j = bits [64 - (j + 1) Q, 64 - j Q)
	if (whole) {
		unsigned long long raw;
		__builtin_memcpy(&raw, idx, 8);
		return __builtin_bswap64(raw);
	}
	const int nbytes = valid == 8 ? Q : (valid * Q + 7) >> 3;
	unsigned long long w = 0;
#pragma unroll
	for (int i = 0; i < Q; i++) {
		const unsigned long long b = i < nbytes ? idx[i] : 0;
		w |= b << (8 * (7 - i));
	}
	return w;
}

} // namespace nnc
