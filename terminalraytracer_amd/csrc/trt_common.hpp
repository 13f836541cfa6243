// trt_common.hpp -- what the kernels of the frame producer share: launch shape of the persistent grid, work-queue
// constants, the LDS image size, the culling-table view, the ISA profile's stage marks and the small streaming
// kernels either side of the render kernel: the queue's start, the ordered mean over a pixel's samples -- one kernel per output kind
// (doubles, RGB8 bytes; the text's is in trt_ansi.hpp), the frame of a launch in blockIdx.y -- and the RGB8 quantisation.
#pragma once

#include "trt_device.hpp"
#include "trt_filter.h"
#include "trt_mean_lanes.h"

namespace trt
{

// threads per workgroup of the persistent kernels: 256 = 4 waves share one LDS image, 4 workgroups per CU
#ifndef TRT_BLOCK
#define TRT_BLOCK 256
#endif
constexpr int kPersistentBlock = TRT_BLOCK;

#if defined(TRT_MARKS) && TRT_MARKS == 2
// -DTRT_MARKS=2: the ISA PROFILE of the shipping kernels (tools/isa_profile.py, tools/build_isa_profile.sh).  A stage boundary
// writes its number to m0 -- which these kernels do not use otherwise; the post-pass checks that -- and the post-pass adds, at
// the head of every basic block, the block's instructions of every kind to lane m0 of one reserved VGPR per kind
// (v_readlane / s_add / v_writelane; s100, s101 and v240... are outside what the kernels allocate).  No stamp sums in
// SGPRs, no counting instantiation: the code profiled is the shipping instantiation's own, up to the scheduling barriers.
#define TRT_MARK_AT(slot)                                        \
    do                                                           \
    {                                                            \
        __builtin_amdgcn_sched_barrier(0);                       \
        asm volatile("s_mov_b32 m0, %0 ; MARK" ::"n"(slot));     \
        __builtin_amdgcn_sched_barrier(0);                       \
    } while (0)
#else
#define TRT_MARK_AT(slot) \
    do                    \
    {                     \
    } while (0)
#endif
constexpr int kProfileKinds = 11, kProfileAt = 40; // counters[kProfileAt + 64 kind + slot]: the ISA profile's sums

// work units (single samples) fetched from the global queue per atomic; a returning atomic per request saturates
// a single queue word (it cost 0.8 ms per frame before pooling)
#ifndef TRT_QUEUE_CHUNK
#define TRT_QUEUE_CHUNK 256
#endif
constexpr unsigned kQueueChunkSamples = TRT_QUEUE_CHUNK;
static_assert(kQueueChunkSamples >= 64, "a chunk must hold the 64 units the lanes of a wave can ask for in one round");
// The queue of a launch is ONE word, or eight (FrameView::queue_shift = 3), one per XCD: the eight L2s keep a contended line coherent
// by passing it around, so a word that only the waves of one XCD ask stays in that XCD's L2 -- a request costs a trip to L2 instead
// of a trip through the fabric, and chunks of half the size stop costing 14 % (profiles/r05/f_ab_log.txt section 16).  Word x hands
// out the chunks (j << shift) + x, j = 0, 1, ..., to the waves of the workgroups x, x + 8, ... -- which the dispatcher deals to the
// XCDs in turn; were it to deal them otherwise, the frame would be the same and only the trips longer.  A wave's FIRST chunk is
// its own: workgroup g, wave k: chunk (j << shift) + (g mod words), j = (g >> shift) * waves per workgroup + k; start_queue_kernel
// starts every word behind those.  The words carry equal work and equal numbers of waves; nobody steals.
constexpr int kQueueXcdShift = 3, kQueueStride = 32;              // words are a 128-byte line apart
constexpr int kQueueLaneWords = (1 << kQueueXcdShift) * kQueueStride; // per lane set (the context's stream, the alternate one)
constexpr int kQueueWords = 2 * kQueueLaneWords;
#ifndef TRT_QUEUE_SMALL_DIV
#define TRT_QUEUE_SMALL_DIV 2
#endif
constexpr unsigned kQueueChunkSmall = TRT_QUEUE_CHUNK / TRT_QUEUE_SMALL_DIV; // the chunk of a launch whose queue has a word per XCD
static_assert(kQueueChunkSmall >= 64, "see kQueueChunkSamples");
#ifndef TRT_CULL_GROUP
#define TRT_CULL_GROUP 8
#endif
constexpr int kCullGroup = TRT_CULL_GROUP; // the culling table is padded to a multiple of this many entries

// FP32 culling table of trt_filter.h on the device
struct CullView
{
    const float *table; // padded to a multiple of kCullGroup entries of {Cx,Cy,Cz,kk}
    int padded;
    double c0x, c0y, c0z;
    float cn, rm;
};

constexpr int kLdsCameraDoubles = 16;                       // basis x,y,z (9) eye (3) -screen_distance (1) basis z * -screen_distance (3)
constexpr int kDirGridDoubles = 14, kPointGridDoubles = 9;  // sizeof(trt_dirgrid) / 8, sizeof(trt_pointgrid) / 8 (asserted in trt_rounds.hpp)

#ifdef TRT_UNIT_RENDER // kernels that are not templates have ONE home among the library's translation units: trt_render.hip
// every word of a launch's queue behind the first chunks of its workgroups (see kQueueStride), written by workgroup (0, 0) of a grid
__device__ __forceinline__ void arm_queue(unsigned int *queue, unsigned grid, unsigned waves_per_group, unsigned shift)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < (1u << shift))
        queue[threadIdx.x * kQueueStride] = (grid > threadIdx.x ? (grid - threadIdx.x + (1u << shift) - 1) >> shift : 0u) * waves_per_group;
}
__global__ void start_queue_kernel(unsigned int *queue, unsigned grid, unsigned waves_per_group, unsigned shift)
{
    arm_queue(queue, grid, waves_per_group, shift);
}
// TRT.c:1063-1066 for frames rendered with samples as work units: pixel = (((0 + s0) + s1) + ...) * (1/spp),
// samples in index order.  The scratch is sample-major, samples[(k*pixels + pixel)*3 + channel], so that for every k
// consecutive threads read consecutive doubles (a pure streaming kernel: spp*24 B read + 24 B written per pixel).
// Over the frames of a launch (a single frame is a launch of one): blockIdx.y is the frame, its scratch is
// samples[((frame * spp + k) * values + i)] and its pixels out[frame * values + i].  Being the last kernel of a launch, it leaves the
// launch's queue ready for a launch of the same shape (start_queue_kernel's job, once per launch: the render kernel that used the queue
// has finished, and the next frame of this context then has no kernel in front of its render kernel).
// WIDE AND DEEP (profiles/r14/a_ordered_mean.md): beside the render kernels of the frames in flight this pass costs the wave slots it
// holds and for how long, so a wave is to make few round trips to memory with much in flight.  A lane owns kMeanGroup consecutive
// values (trt_mean_lanes.h: the groups, then a lane per value they leave) and issues the loads of kMeanDeep samples -- one 16-byte
// load each -- before the first add; the adds follow in sample order as the loads land.  spp is whole blocks of kMeanDeep, then a
// remainder a sample at a time; the reference's spp = 10 is two blocks.  Two values x five samples is 30 VGPRs: a wave fits into the
// 32 registers that four plain render waves of 119 leave a SIMD, which deeper and wider shapes (50, 54) do not, and config 5 pays for.
// Frame, values and out are 8-byte aligned and no more: the 16-byte accesses are the hardware's unaligned ones, as
// reduce_samples_rgb8's are.
#ifndef TRT_REDUCE_DEEP
#define TRT_REDUCE_DEEP 5
#endif
#ifndef TRT_REDUCE_NT
#define TRT_REDUCE_NT 0 // 1: non-temporal loads of the scratch (A/B in profiles/r14/a_ordered_mean.md)
#endif
constexpr int kMeanGroup = TRT_MEAN_GROUP, kMeanDeep = TRT_REDUCE_DEEP;

__device__ __forceinline__ double mean_sample(const double *p)
{
#if TRT_REDUCE_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

__global__ __launch_bounds__(256) void reduce_samples_kernel(const double *samples, double *out, long values, int spp, double inv_spp,
                                                             unsigned int *queue, unsigned grid, unsigned waves_per_group, unsigned shift)
{
    arm_queue(queue, grid, waves_per_group, shift);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int owned = trt_mean_lane_values(values, i);
    if (owned == 0)
        return;
    const long v = (long)trt_mean_lane_first(values, i);
    const double *s = samples + (size_t)blockIdx.y * (size_t)spp * (size_t)values + v; // sample k of the lane's values: s + k * values
    double *to = out + (size_t)blockIdx.y * (size_t)values + v;
    if (owned == kMeanGroup)
    {
        double mean[kMeanGroup];
#pragma unroll
        for (int g = 0; g < kMeanGroup; g++)
            mean[g] = 0.0;
        int k = 0;
        for (; k + kMeanDeep <= spp; k += kMeanDeep)
        {
            double block[kMeanDeep][kMeanGroup];
#pragma unroll
            for (int d = 0; d < kMeanDeep; d++, s += values)
#pragma unroll
                for (int g = 0; g < kMeanGroup; g++)
                    block[d][g] = mean_sample(s + g);
#pragma unroll
            for (int d = 0; d < kMeanDeep; d++) // in sample order
#pragma unroll
                for (int g = 0; g < kMeanGroup; g++)
                    mean[g] += block[d][g];
        }
        for (; k < spp; k++, s += values)
#pragma unroll
            for (int g = 0; g < kMeanGroup; g++)
                mean[g] += mean_sample(s + g);
#pragma unroll
        for (int g = 0; g < kMeanGroup; g++)
            to[g] = mean[g] * inv_spp;
        return;
    }
    double mean = 0.0; // a value behind the groups
    for (int k = 0; k < spp; k++, s += values)
        mean += mean_sample(s);
    *to = mean * inv_spp;
}

// (int)(c*255) per channel, TRT.c:1157-1163
__global__ void quantize_kernel(const double *px, long n_values, unsigned char *rgb)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_values)
        rgb[i] = (unsigned char)d2i(px[i] * 255);
}

// The ordered mean and the emitter's cast in ONE pass, for the hosts whose only consumer of a frame is the emitter: per value what
// reduce_samples_kernel and quantize_kernel compute one after the other -- (unsigned char)d2i((mean * inv_spp) * 255), the mean summed
// from 0.0 in sample order -- without the 24 B per pixel of doubles written and read back in between.  A lane owns kRgb8Group
// consecutive values: per k it reads them as 32 consecutive bytes of the scratch (16-byte loads) and at the end it stores them as ONE
// aligned 32-bit word, so that a wave's store covers 256 consecutive bytes instead of 64.  `out` may have any byte alignment: the
// groups start at the first 4-aligned ADDRESS, `head` = (-out) mod 4 values in (all of them, if there are fewer), and the up to three
// values in front of the groups and the up to three behind them have a lane and a single-byte store each.  Lane i: group i while
// i < groups, then the head's values, then the tail's; the grid has groups + head + tail lanes (rgb8_lanes), rounded up to workgroups.
constexpr int kRgb8Group = 4;

__host__ __device__ inline long rgb8_head(const unsigned char *out, long values)
{
    const long head = (long)((4 - ((unsigned long long)out & 3)) & 3);
    return head < values ? head : values;
}
// lanes of a frame of `values` values that starts `head` values in front of a 4-aligned address
__host__ __device__ inline long rgb8_lanes(long values, long head)
{
    return (values - head) / kRgb8Group + head + (values - head) % kRgb8Group;
}

__device__ __forceinline__ unsigned rgb8_byte(double mean, double inv_spp)
{
    return (unsigned)(unsigned char)d2i((mean * inv_spp) * 255); // TRT.c:1065, then TRT.c:1157-1163
}

// one frame's lane `i`: samples[k * values + v] -> out[v]
__device__ __forceinline__ void reduce_samples_rgb8(const double *samples, unsigned char *out, long values, int spp, double inv_spp, long i)
{
    const long head = rgb8_head(out, values);
    const long groups = (values - head) / kRgb8Group;
    if (i < groups)
    {
        const long v = head + i * kRgb8Group;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
#pragma unroll 4 // the loads of four samples in flight per lane; the sums stay in sample order
        for (int k = 0; k < spp; k++)
        {
            const double *s = samples + ((long)k * values + v);
            m0 += s[0];
            m1 += s[1];
            m2 += s[2];
            m3 += s[3];
        }
        const unsigned word = rgb8_byte(m0, inv_spp) | rgb8_byte(m1, inv_spp) << 8 | rgb8_byte(m2, inv_spp) << 16 | rgb8_byte(m3, inv_spp) << 24;
        *reinterpret_cast<unsigned *>(out + v) = word; // (out + head) is 4-aligned, and so is every group behind it
        return;
    }
    const long j = i - groups; // the values the groups leave: the head's, then the tail's
    const long v = j < head ? j : head + groups * kRgb8Group + (j - head);
    if (v >= values)
        return;
    double mean = 0.0;
    for (int k = 0; k < spp; k++)
        mean += samples[(long)k * values + v];
    out[v] = (unsigned char)rgb8_byte(mean, inv_spp);
}

// ... as the last kernel of a launch, in reduce_samples_kernel's place: blockIdx.y is the frame, and it leaves the queue ready in the
// same way.  Frame b's bytes start at out + b * values, which is 4-aligned for no b in general: every frame has a head and a tail of its
// own.  A single frame's grid has exactly its lanes; that of several frames the most lanes any alignment needs (at most values / 4
// groups, three values in front, three behind; a frame's spare lanes find nothing to do).
__global__ __launch_bounds__(256) void reduce_samples_rgb8_kernel(const double *samples, unsigned char *out, long values, int spp, double inv_spp,
                                                                  unsigned int *queue, unsigned grid, unsigned waves_per_group, unsigned shift)
{
    arm_queue(queue, grid, waves_per_group, shift);
    reduce_samples_rgb8(samples + (size_t)blockIdx.y * (size_t)spp * (size_t)values, out + (size_t)blockIdx.y * (size_t)values, values, spp, inv_spp,
                        (long)blockIdx.x * blockDim.x + threadIdx.x);
}

#endif // TRT_UNIT_RENDER

} // namespace trt
