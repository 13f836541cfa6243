/*
 * trt_mean_lanes.h -- which lane of the ordered mean's doubles pass owns which values of a frame (host + device, plain C).
 *
 * reduce_samples_kernel (trt_common.hpp) gives a lane TRT_MEAN_GROUP consecutive values, so that a sample of them is ONE load and
 * their means ONE store.  A frame of `values` values has values / TRT_MEAN_GROUP such groups, lane i the values
 * [i, i + 1) * TRT_MEAN_GROUP, and behind them a lane for each of the values % TRT_MEAN_GROUP values the groups leave, as the bytes
 * form has (rgb8_lanes).  The kernel, the launch that sizes its grid (trt_render.hip) and the host check (tests/mean_lanes_check.c)
 * compile this one map.
 */
#ifndef TRT_MEAN_LANES_H
#define TRT_MEAN_LANES_H

#if defined(__HIPCC__) || defined(__HIP__)
#define TRT_MEAN_HD __host__ __device__ __forceinline__
#else
#define TRT_MEAN_HD static inline
#endif

#ifndef TRT_MEAN_GROUP
#define TRT_MEAN_GROUP 2 /* values per lane: 16 bytes a load */
#endif

/* lanes of a frame of `values` values */
TRT_MEAN_HD long long trt_mean_lanes(long long values) { return values / TRT_MEAN_GROUP + values % TRT_MEAN_GROUP; }

/* how many values lane `lane` owns: TRT_MEAN_GROUP, one (a tail lane) or none (a spare lane of the last workgroup) */
TRT_MEAN_HD int trt_mean_lane_values(long long values, long long lane)
{
    const long long groups = values / TRT_MEAN_GROUP;
    return lane < groups ? TRT_MEAN_GROUP : lane < groups + values % TRT_MEAN_GROUP ? 1 : 0;
}

/* the first of them */
TRT_MEAN_HD long long trt_mean_lane_first(long long values, long long lane)
{
    const long long groups = values / TRT_MEAN_GROUP;
    return lane < groups ? lane * TRT_MEAN_GROUP : groups * TRT_MEAN_GROUP + (lane - groups);
}

#endif
