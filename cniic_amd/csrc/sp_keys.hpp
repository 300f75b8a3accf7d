// sp_keys.hpp -- a colour key (0xRRGGBB) as (super-cell bucket, colour inside the bucket) and back: the numbering of the pixel
// partition (k_points.hip), which the persistent K-means reads the histogram's staged colours in (k_kmeans_persist.hip).
// 512 buckets r[7:5] g[7:5] b[7:5]; a bucket's 64 colour cells are cells 64 bucket .. 64 bucket + 63 of the K-means (cell_of).
#pragma once
#include <cstdint>

namespace cniic {

__device__ __forceinline__ uint32_t sp_bucket(uint32_t key) {
    return (((key >> 21) & 7u) << 6) | (((key >> 13) & 7u) << 3) | ((key >> 5) & 7u);
}
// colour inside its super-cell, cell-major: cell within the super-cell (cell_of's low 6 bits) << 9 | colour within the cell
__device__ __forceinline__ uint32_t sp_bin(uint32_t key) {
    const uint32_t r = (key >> 16) & 31u, g = (key >> 8) & 31u, b = key & 31u;
    return ((r >> 3) << 13) | ((g >> 3) << 11) | ((b >> 3) << 9) | ((r & 7u) << 6) | ((g & 7u) << 3) | (b & 7u);
}
__device__ __forceinline__ uint32_t sp_key(uint32_t bucket, uint32_t bin) {
    const uint32_t r = (((bucket >> 6) & 7u) << 5) | (((bin >> 13) & 3u) << 3) | ((bin >> 6) & 7u);
    const uint32_t g = (((bucket >> 3) & 7u) << 5) | (((bin >> 11) & 3u) << 3) | ((bin >> 3) & 7u);
    const uint32_t b = ((bucket & 7u) << 5) | (((bin >> 9) & 3u) << 3) | (bin & 7u);
    return (r << 16) | (g << 8) | b;
}

}  // namespace cniic
