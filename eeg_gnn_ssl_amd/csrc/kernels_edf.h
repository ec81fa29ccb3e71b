// EDF payload -> physical signals on the device (the reference's `getEDFsignals`, data/data_utils.py, which goes through EDFlib's
// readSignal): the int16 samples of the selected signals of every data record, scaled to float64 (or rounded once to float32) and laid
// out channel-major.
//
// The payload is `num_records` records of R int16 each; record r holds, for selected channel c, n samples at int16 index
// r * R + off[c] .. + n.  Output row c, sample t = r * n + j:
//     out[c * out_stride + t] = gain[c] * (offset[c] + (double)d),   d = payload[r * R + off[c] + j]
// EDFlib's arithmetic with gain = (pmax - pmin) / (dmax - dmin), offset = pmax / gain - dmax computed once on the host in float64: ONE
// float64 add, then ONE float64 multiply, each correctly rounded.  (a + b) * c has no fused form and the function is compiled with
// contraction off, so nothing re-associates them; the float32 output is that float64 value rounded once on the store.
//
// Tiling.  A workgroup of kEdfThreads threads writes kEdfTile consecutive samples of ONE output row: thread i writes samples
// t0 + i + k * kEdfThreads, so every store instruction of a wave covers 64 consecutive elements (256 / 512 contiguous bytes, the
// full-rate store shape) whatever n is; a tile may straddle any number of record boundaries.  The record of a sample costs one 64-bit
// division per WORKGROUP (t0 / n) and one 32-bit division by the uniform n per sample.  The loads are one int16 per lane: the lanes of
// a wave read consecutive int16 of a run, i.e. one or two 128-byte lines per instruction, and they are 1/5 (float64) or 1/3
// (float32) of the kernel's bytes; the four loads of a thread are issued before its first store.  No LDS, no atomics.
//
// The rule of the loads: a lane reads the two bytes of its own sample and nothing else.  No access is wider than the sample, so the
// parity of R, of off[c] and of the payload address never matters, a run's first and last values are never fetched together with a
// neighbouring signal's, and no byte at or behind payload + 2 * num_records * R (<= payload_bytes, checked by the host) is ever
// touched -- nor one in front of `payload`.  All index arithmetic is 64-bit (r * R passes 2^31); the host guarantees n <= 2^30,
// off[c] + n <= R, out_stride >= num_records * n.
//
// The per-channel constants travel BY VALUE in the kernel argument (EdfChannels, at most kEdfMaxChannels = the project's num_nodes
// limit): no device table, no copy in front of the launch.
#pragma once
#include <cstdint>

#include "common.h"

namespace eeg {

constexpr int kEdfThreads = 256;
constexpr int kEdfPerThread = 4;
constexpr int kEdfTile = kEdfThreads * kEdfPerThread;   // 1024 samples of one row per workgroup
constexpr int kEdfMaxChannels = 32;                     // EEG_EDF_MAX_CHANNELS
constexpr long long kEdfMaxN = 1ll << 30;               // samples per record of a selected signal (an 8-digit header field stays below)

struct EdfChannels {
    double gain[kEdfMaxChannels];
    double offset[kEdfMaxChannels];
    long long off[kEdfMaxChannels];                     // first int16 of the channel inside a record
};

template <typename T, int PER = kEdfPerThread>
__global__ void __launch_bounds__(kEdfThreads)
edf_decode_kernel(const int16_t* __restrict__ payload, long long num_records, long long R, long long n, EdfChannels ch, T* __restrict__ out,
                  long long out_stride) {
#pragma clang fp contract(off)
    const int c = blockIdx.y;
    const long long L = num_records * n;
    const long long t0 = (long long)blockIdx.x * (kEdfThreads * PER);
    const long long r0 = t0 / n;                                         // the tile's first record (workgroup-uniform)
    const unsigned j0 = (unsigned)(t0 - r0 * n), nn = (unsigned)n;       // j0 < n <= 2^30: j0 + i stays below 2^31
    const double gain = ch.gain[c], offset = ch.offset[c];
    const int16_t* run = payload + ch.off[c];
    T* row = out + (long long)c * out_stride;
    int16_t d[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const unsigned i = threadIdx.x + (unsigned)k * kEdfThreads;
        d[k] = 0;
        if (t0 + i < L) {
            const unsigned q = j0 + i, dr = q / nn, j = q - dr * nn;
            d[k] = run[(r0 + dr) * R + j];
        }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const unsigned i = threadIdx.x + (unsigned)k * kEdfThreads;
        if (t0 + i < L) row[t0 + i] = (T)(gain * (offset + (double)d[k]));
    }
}

}  // namespace eeg
