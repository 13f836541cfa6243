/* mean_lanes_check.c -- csrc/trt_mean_lanes.h, the lane map of the ordered mean's doubles pass, compiled for the host: for every frame
 * of 1 .. 399 values, walk the lanes of the grid the launch would make (whole workgroups of 64, and one workgroup more) and count who
 * owns what.  Every value has exactly one lane; a group lies inside the frame and starts at a multiple of the group; no lane behind
 * trt_mean_lanes owns anything.  tests/test_ordered_mean_wide.py builds and runs it. */
#include <stdio.h>
#include <string.h>

#include "trt_mean_lanes.h"

#define MOST 399

int main(void)
{
    for (long long values = 1; values <= MOST; values++)
    {
        int owners[MOST];
        memset(owners, 0, sizeof owners);
        const long long lanes = trt_mean_lanes(values), grid = (lanes + 63) / 64 * 64 + 64;
        if (lanes < (values + TRT_MEAN_GROUP - 1) / TRT_MEAN_GROUP || lanes > values)
            return printf("values %lld: %lld lanes\n", values, lanes), 1;
        for (long long lane = 0; lane < grid; lane++)
        {
            const int n = trt_mean_lane_values(values, lane);
            const long long first = trt_mean_lane_first(values, lane);
            if (n != 0 && n != 1 && n != TRT_MEAN_GROUP)
                return printf("values %lld lane %lld: owns %d\n", values, lane, n), 1;
            if (lane >= lanes && n != 0)
                return printf("values %lld: spare lane %lld owns %d\n", values, lane, n), 1;
            if (lane < lanes && n == 0)
                return printf("values %lld: lane %lld of %lld owns nothing\n", values, lane, lanes), 1;
            if (n && (first < 0 || first + n > values))
                return printf("values %lld lane %lld: [%lld, %lld) leaves the frame\n", values, lane, first, first + n), 1;
            if (n == TRT_MEAN_GROUP && first % TRT_MEAN_GROUP)
                return printf("values %lld lane %lld: a group at %lld\n", values, lane, first), 1;
            for (int g = 0; g < n; g++)
                owners[first + g]++;
        }
        for (long long v = 0; v < values; v++)
            if (owners[v] != 1)
                return printf("values %lld: value %lld has %d lanes\n", values, v, owners[v]), 1;
    }
    printf("mean_lanes_check: ok (group %d)\n", TRT_MEAN_GROUP);
    return 0;
}
