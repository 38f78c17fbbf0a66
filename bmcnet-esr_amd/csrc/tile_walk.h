// The persistent workgroups' walk over a launch's tile list, shared by the matrix-core kernels (conv.hip, conv_bf.hip,
// conv1.hip, conv1p.hip, wino.hip, wino4.hip, chain.hip): which tiles a workgroup visits, and the tile index as digits.
#pragma once

constexpr int NUM_XCD = 8;      // accelerator dies of the device, each with its own L2

// Workgroup blockIdx.x visits the tiles first, first + stride, ... below hi (count of them); the load pipelines run ahead
// of the MFMA pipelines across tile boundaries, so only the very first tile of a workgroup pays load latency.
// XCD-aware: workgroups are dealt round-robin over the XCDs (blockIdx % 8 shares an L2), so give each XCD one contiguous
// eighth of the tile list and let its workgroups sweep it side by side -- neighbouring tiles (shared halo rows/columns)
// then meet in the same L2 while hot.  Speed only; any placement is correct.
struct TileWalk { int first, hi, stride, count; };
__device__ __forceinline__ TileWalk tile_walk(int ntiles) {
    const bool xcd_map = (gridDim.x % NUM_XCD) == 0 && ntiles >= (int)gridDim.x;
    const int xcd = blockIdx.x % NUM_XCD, xj = blockIdx.x / NUM_XCD, per_x = gridDim.x / NUM_XCD;
    const int t_lo = xcd_map ? (int)((long long)ntiles * xcd / NUM_XCD) : 0;
    const int t_hi = xcd_map ? (int)((long long)ntiles * (xcd + 1) / NUM_XCD) : ntiles;
    const int t_first = xcd_map ? t_lo + xj : (int)blockIdx.x;
    const int t_stride = xcd_map ? per_x : (int)gridDim.x;
    const int my_tiles = t_first < t_hi ? (t_hi - t_first + t_stride - 1) / t_stride : 0;     // block-uniform
    return TileWalk{t_first, t_hi, t_stride, my_tiles};
}

// Tile index -> digits is a mixed-radix decode: one integer division per digit, ~40 VALU instructions each, that every
// user of a tile's coordinates (loaders, epilogue) would pay per tile beside the MFMAs.  A workgroup visits first,
// first + stride, ...: decode the first tile and the stride once, then advance digit-wise with carries.
// Three digits below the image: (channel tile, tile column, tile row, image).
struct Tile3 { int nt, tx, ty, b; };
__device__ __forceinline__ Tile3 tile_decode(int t, int ntn, int tiles_x, int tiles_y) {
    Tile3 it;
    it.nt = t % ntn; t /= ntn;
    it.tx = t % tiles_x; t /= tiles_x;
    it.ty = t % tiles_y;
    it.b = t / tiles_y;
    return it;
}
__device__ __forceinline__ Tile3 tile_advance(Tile3 it, const Tile3& stp, int ntn, int tiles_x, int tiles_y) {
    it.nt += stp.nt;
    if (it.nt >= ntn) { it.nt -= ntn; ++it.tx; }
    it.tx += stp.tx;
    if (it.tx >= tiles_x) { it.tx -= tiles_x; ++it.ty; }
    it.ty += stp.ty;
    if (it.ty >= tiles_y) { it.ty -= tiles_y; ++it.b; }
    it.b += stp.b;
    return it;
}
// Two digits below the image: (channel tile, position of the tile in its image, image) -- kernels whose tiles are runs
// of an image's flattened pixel or tile list (per_img of them).
struct Tile2 { int nt, pt, b; };
__device__ __forceinline__ Tile2 tile_decode(int t, int ntn, int per_img) {
    Tile2 it;
    it.nt = t % ntn; t /= ntn;
    it.pt = t % per_img;
    it.b = t / per_img;
    return it;
}
__device__ __forceinline__ Tile2 tile_advance(Tile2 it, const Tile2& stp, int ntn, int per_img) {
    it.nt += stp.nt;
    if (it.nt >= ntn) { it.nt -= ntn; ++it.pt; }
    it.pt += stp.pt;
    if (it.pt >= per_img) { it.pt -= per_img; ++it.b; }
    it.b += stp.b;
    return it;
}
