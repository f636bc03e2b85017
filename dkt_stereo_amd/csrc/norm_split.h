// norm_split.h -- blocks per plane of the instance norm's statistics launches (norm.hip forward, norm_train.hip backward):
// several blocks per plane so that a few large planes still fill the device.
#pragma once

#define NORM_SPLIT_MAX 64

static inline int norm_split(int planes, long HW) {
    int S = (2048 + planes - 1) / planes;          // ~2048 blocks in flight
    const long max_split = (HW + 4095) / 4096;      // at least 4096 elements per block
    if (S > max_split) S = (int)max_split;
    if (S > NORM_SPLIT_MAX) S = NORM_SPLIT_MAX;
    if (S < 1) S = 1;
    return S;
}
