// ds_kernels.hh — launchers for the MI355X pyramid kernels (ds_kernels.hip).
//
// Three kernels cover the reference's two hot loops
// (src/streaming/downsampler.cpp):
//   * cascade   — scale_image<T> (:139-206) applied 1..4 times in one pass:
//                 each wave reads a 2^NL-row base tile once and writes every
//                 level of the run; odd edges replicated per level.
//   * xy_generic — one scale_image<T> level, one output pixel per lane; used
//                 by the general state machine and for frames narrower than
//                 one vector load.
//   * zpair     — average_two_frames<T> (:208-246), out = f(earlier, current).
//   * volume    — both of the above fused for pyramids whose levels halve XY
//                 and Z (3-D stacks): 2^NL planes x 2^NL rows per wave, every
//                 level written from registers.
//   * zrun      — zpair applied 1..3 times in one pass over a batch of whole
//                 plane groups (levels that halve Z alone): 2^NL planes per
//                 wave, every level written from registers.
#pragma once

#include <hip/hip_runtime.h>

#include "ds_plan.hh" // LevelOut, TiledOut, the geometry helpers and the launch plans

namespace aqz {

// Fused multi-level XY reduction of `n_frames` frames (frame i at
// src + i*src_frame_elems).  n_out in [1, kMaxFusedLevels].
hipError_t launch_cascade(int dtype, int method, const void* src, uint64_t src_frame_elems,
                          uint32_t W, uint32_t H, const LevelOut* outs, int n_out,
                          uint32_t n_frames, hipStream_t stream);

// launch_cascade with every level written chunk-tiled from registers: one
// kernel, whose trailing waves zero-fill the tile overhang past the frame
// (plus one flag clear per level whose tiles do not hold whole wave blocks).
// touts[i].nonzero then holds n_frames * n_tiles * max(1, slots) bytes.
// outs[i] gives level i's geometry; its ptr, when non-null, also receives the
// level row-major (the input of a following launch).  Same geometry rules as
// launch_cascade.
// `tbase`, when non-null: the input level itself (W x H) goes out the same
// way from the same kernel — the block each wave has loaded, stored as tiles
// before the first reduction — with its own tile shape, flags and lattice.
hipError_t launch_cascade_tiled(int dtype, int method, const void* src,
                                uint64_t src_frame_elems, uint32_t W, uint32_t H,
                                const LevelOut* outs, const TiledOut* touts, int n_out,
                                uint32_t n_frames, hipStream_t stream,
                                const TiledOut* tbase = nullptr);

// Fused 2x2x2 (XY reduce, then Z pair) over `n_planes` consecutive planes for
// pyramids whose levels all halve both XY and Z; n_planes must be a multiple
// of 2^n_out, n_out in [1, kMaxVolumeLevels].  Level L receives
// n_planes >> L frames.
hipError_t launch_volume(int dtype, int method, const void* src, uint64_t src_frame_elems,
                         uint32_t W, uint32_t H, const LevelOut* outs, int n_out,
                         uint32_t n_planes, hipStream_t stream);

// launch_volume with every level written chunk-tiled from registers, plane k
// of level L as frame k of touts[L-1] (n_planes >> L planes: that many
// frame_offsets entries for a chunk lattice).  One kernel; its first waves
// zero-fill the tile overhang; touts[i].nonzero, when set, is cleared by a
// fill queued first and holds one byte per tile per emitted plane.  outs[i]
// gives level i's geometry; its ptr, when non-null, also receives the level
// row-major (the input of a following launch).
hipError_t launch_volume_tiled(int dtype, int method, const void* src, uint64_t src_frame_elems,
                               uint32_t W, uint32_t H, const LevelOut* outs,
                               const TiledOut* touts, int n_out, uint32_t n_planes,
                               hipStream_t stream);

// One XY level, any width/alignment.
// (The dtype-dispatching launchers are routed by ds_dispatch.cpp to the build
// shard of ds_kernels.hip that holds the dtype's kernels; the four above are
// planned there first, ds_plan.hh.)
hipError_t launch_xy_generic(int dtype, int method, const void* src, uint64_t src_frame_elems,
                             uint32_t w, uint32_t h, const LevelOut& out, uint32_t n_frames,
                             hipStream_t stream);

// out[i] = reduce2(earlier[i], current[i]) over n elements; `out` may alias
// either input.  16-byte vectors when all pointers are aligned, else scalar.
hipError_t launch_zpair(int dtype, int method, void* out, const void* earlier,
                        const void* current, uint64_t n, hipStream_t stream);

// 1..kMaxZLevels levels that halve Z alone, in one pass: `planes` frames of
// `elems` elements (src_frame_elems apart) are paired down n_out times in
// registers; level j (1-based) receives planes >> j frames at
// outs[j-1].ptr + k * outs[j-1].frame_elems (its w and h are not read), each
// reduce2(earlier, current) of level j-1's frames 2k and 2k+1.  Any element
// count and element-aligned pointer; `planes` a multiple of 2^n_out.  Planned
// by plan_zrun (ds_plan.hh), whose refusals come back as
// hipErrorInvalidValue before anything is queued.
hipError_t launch_zrun(int dtype, int method, const void* src, uint64_t src_frame_elems,
                       uint64_t elems, const LevelOut* outs, int n_out, uint32_t planes,
                       hipStream_t stream);

// launch_zrun over planes of W x H elements with every level written
// chunk-tiled from registers, plane k of level j as frame k of touts[j-1]
// (planes >> j planes: that many frame_offsets entries for a chunk lattice),
// each level in its own tile shape.  One kernel; its first waves zero-fill
// the tile overhang; touts[i].nonzero, when set, is cleared by a fill queued
// first and holds one byte per tile per emitted plane.  outs[i].ptr, when
// non-null, also receives the level row-major (the input of a following
// launch).  Planned by plan_zrun_tiled (ds_plan.hh).
hipError_t launch_zrun_tiled(int dtype, int method, const void* src, uint64_t src_frame_elems,
                             uint32_t W, uint32_t H, const LevelOut* outs,
                             const TiledOut* touts, int n_out, uint32_t planes,
                             hipStream_t stream);

// Chunk tiling of one W x H frame (array.cpp:507-622 / chunk.cpp:17-58):
// transpose_frame (array.cpp:488-504): `dst` (cols x rows, row-major)
// receives the transpose of `src` (rows x cols, row-major).
hipError_t launch_transpose(int dtype, const void* src, uint32_t rows, uint32_t cols, void* dst,
                            hipStream_t stream);

// `dst` receives n_tiles x tile_rows x tile_cols elements, tile-major,
// zero-padded; `nonzero[t]` (device, one u32 per tile, cleared here) is set
// when tile t holds any nonzero byte.
hipError_t launch_tile_frame(int dtype, const void* src, uint32_t W, uint32_t H,
                             uint32_t tile_rows, uint32_t tile_cols, void* dst,
                             uint32_t* nonzero, hipStream_t stream);

// Same tiling with one flag byte per (tile, slice): slice_flags holds
// n_tiles * tile_slices(tile_rows, tile_cols) bytes (tile-major), written
// without atomics or a pre-clear; a tile is nonzero iff any of its slices is.
hipError_t launch_tile_frame_sliced(int dtype, const void* src, uint32_t W, uint32_t H,
                                    uint32_t tile_rows, uint32_t tile_cols, void* dst,
                                    uint8_t* slice_flags, hipStream_t stream);

} // namespace aqz
