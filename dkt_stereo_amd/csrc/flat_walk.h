// flat_walk.h -- one launch over a LIST of tensors of arbitrary sizes (ema.hip, optim.hip).
//
// A device table of count + 1 exclusive prefix offsets flattens the list, and the grid strides over fixed tiles of
// THREADS * ITEMS elements of that flat range, so whatever belongs to a tile does not depend on the grid.  A tile that lies
// inside one tensor (all but the few that straddle a boundary) is handed over whole: the kernel reads its base pointers
// once and keeps ITEMS loads of each operand in flight per thread.  A straddling tile is walked element by element, each
// thread taking its elements in increasing order.  The accesses are dwords, coalesced across the wave: a tensor boundary
// may fall on any element, so no wider access is aligned in general.
//
// absmax (optional): max |value| per tensor as an integer atomicMax on the bit patterns of non-negative floats -- max is
// order-independent, so the result does not depend on the schedule.  A whole tile takes the block's maximum first (one
// atomic per tile); a straddling thread flushes its running maximum whenever its tensor advances.
#pragma once
#include "wave_reduce.h"

// the tensor holding flat element e: the largest k with off[k] <= e (empty tensors have off[k] == off[k+1] and are skipped)
__device__ __forceinline__ int flat_tensor_of(const long *__restrict__ off, int count, long e) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The tile loop.  Callbacks, inlined:
//   unsigned inside(k, base, end)   tile [base, end) lies inside tensor k; thread t owns base + j * THREADS + t, j < ITEMS
//   unsigned element(k, i, j)       element i of tensor k, the thread's item j < ITEMS, on a straddling tile
//   void     done(tile)             after either path, by every thread
// inside / element return the bit pattern of |value| for absmax (anything when absmax is null).  `red`: THREADS / 64
// unsigneds of LDS (unused when absmax is null).
template <int THREADS, int ITEMS, class Inside, class Element, class Done>
__device__ __forceinline__ void flat_walk(const long *__restrict__ off, int count, unsigned *__restrict__ absmax, unsigned *red,
                                          Inside inside, Element element, Done done) {
    constexpr int TILE = THREADS * ITEMS;
    const long total = off[count];
    const long tiles = (total + TILE - 1) / TILE;
    const int tid = threadIdx.x;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long base = tile * TILE;
        const long end = base + TILE < total ? base + TILE : total;
        int k = flat_tensor_of(off, count, base);
        if (off[k + 1] >= end) {
            unsigned m = inside(k, base, end);
            if (absmax) {
                m = block_max<THREADS / 64>(m, red);
                if (tid == 0) atomicMax(absmax + k, m);
            }
        } else {
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const long e = base + j * THREADS + tid;
                if (e >= end) break;
                while (e >= off[k + 1]) {
                    if (absmax && m) atomicMax(absmax + k, m);
                    m = 0;
                    ++k;
                }
                const unsigned u = element(k, e - off[k], j);
                m = u > m ? u : m;
            }
            if (absmax && m) atomicMax(absmax + k, m);
        }
        done(tile);
    }
}

// Blocks of a flat_walk launch: 8 blocks of 4 waves per CU, the CU's full occupancy, and never more blocks than tiles
// (tiles < 0: not known on the host).
static inline long flat_walk_blocks(long tiles) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    long blocks = (long)cus * 8;
    if (tiles >= 0 && blocks > tiles) blocks = tiles;
    return blocks < 1 ? 1 : blocks;
}
