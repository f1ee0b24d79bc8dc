// gpsiq_stream.h -- the device side of what the span stages' kernels (gpsiq_filter, gpsiq_cfilter, gpsiq_resample, gpsiq_mix) do alike
// with a stream of interleaved I,Q samples, int8 or int16, stated once: read a sample as one dword, the x(m) of the span contracts,
// round and clamp an int32 sum, write a sample, and add a workgroup's count of clamped elements into the call's counter.
// A piece lives here only in a form that leaves every kernel's instruction stream as it was (scripts/row_loop_listing.py --hashes;
// profiles/stream_header_kernel_hashes.txt).  Where no form did, the site keeps its own text: pack_stream (gpsiq_pack_kernels.hip) and
// agc_apply (gpsiq_agc_kernels.hip) end in count_clipped's steps written out in place.  What is another arithmetic stays with its
// stage: rs_finish of the resampler (two row sums and a weight) and the 64-bit finish of the mixer (a run-time qmax).
#ifndef GPSIQ_STREAM_H
#define GPSIQ_STREAM_H

#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"

namespace gpsiq {
namespace stream {

// four dwords: a 16-byte load, and an operand or the accumulator of v_mfma_i32_16x16x64_i8 (the matrix kernels of the acquisition
// search, the two filters and the spectrum)
typedef int i32x4 __attribute__((ext_vector_type(4)));

// sample m of the stream as one dword: I in the low half, Q in the high half, each sign-extended to 16 bits
template <int FMT>
__device__ __forceinline__ uint32_t load_pair(const uint8_t *base, int64_t m)
{
    if (FMT == GPSIQ_SC16) return *reinterpret_cast<const uint32_t *>(base + (uint64_t) m * 4);
    const uint32_t v = *reinterpret_cast<const uint16_t *>(base + (uint64_t) m * 2);
    return ((uint32_t) (int32_t) (int8_t) (v & 0xffu) & 0xffffu) | ((uint32_t) (int32_t) (int8_t) (v >> 8) << 16);
}

// x(m) of the contract: the span, the head before it, zeros before that and where there is no head
template <int FMT>
__device__ __forceinline__ uint32_t sample_at(const uint8_t *src, const uint8_t *head, int64_t m, int nsamp, int ntaps)
{
    if (m >= 0) return m < (int64_t) nsamp ? load_pair<FMT>(src, m) : 0u;
    return head && m >= -(int64_t) (ntaps - 1) ? load_pair<FMT>(head, (int64_t) (ntaps - 1) + m) : 0u;
}

// y = floor((acc + 2^(shift-1)) / 2^shift), clamped to +-QMAX; clipped counts the elements the clamp changed
template <int OUT>
__device__ __forceinline__ int finish(int acc, int shift, unsigned &clipped)
{
    constexpr int QMAX = OUT == GPSIQ_SC08 ? 127 : 32767;
    const int64_t half = shift ? (int64_t) 1 << (shift - 1) : 0;
    const int64_t y = ((int64_t) acc + half) >> shift;
    const int64_t c = y < -QMAX ? -QMAX : y > QMAX ? QMAX : y;
    clipped += c != y;
    return (int) c;
}

template <int OUT>
__device__ __forceinline__ void store_sample(uint8_t *dst, uint64_t j, int i, int q)
{
    if (OUT == GPSIQ_SC16) *reinterpret_cast<uint32_t *>(dst + j * 4) = ((uint32_t) i & 0xffffu) | ((uint32_t) q << 16);
    else *reinterpret_cast<uint16_t *>(dst + j * 2) = (uint16_t) (((uint32_t) i & 0xffu) | (((uint32_t) q & 0xffu) << 8));
}

// The count of a workgroup of THREADS threads: per wave, then per workgroup; one atomic of the workgroup if it clamped anything.
// Integer addition: the order of arrival does not matter.  Every thread of the workgroup arrives here.  (The partial counts, one
// per wave, are the filter, complex filter and resampler kernels' only static LDS: four of them, 32 bytes, so the dynamic region
// behind them, which the matrix kernels read 16 bytes at a time, stays 16-byte aligned.)
template <int THREADS>
__device__ __forceinline__ void count_clipped(unsigned long long clipped, unsigned long long *count)
{
    for (int off = 32; off >= 1; off >>= 1) clipped += __shfl_xor(clipped, off, 64);
    __shared__ unsigned long long part[THREADS / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = clipped;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (int k = 0; k < THREADS / 64; ++k) sum += part[k];
        if (sum) atomicAdd(count, sum);
    }
}

}  // namespace stream
}  // namespace gpsiq
#endif
