/*
 * fplroi.h - C ABI of libfplroi.so: the region of interest (flypylib_amd/roi.py: BlockRoi, DVID's
 * runs of blocks) on the GPU - the uint8 mask of a box, point queries, voxel counts of boxes - and
 * the cut-and-normalise of a training cube.  The specification is roi.py's numpy; every entry
 * point reproduces it bit for bit.
 *
 * Conventions of the side libraries: 0 on success, else non-zero with the text in
 * fplr_last_error() (thread-local); no C++ exception crosses the boundary; every argument is
 * checked before anything is launched.  `stream` is a hipStream_t (NULL: the default stream);
 * every call is stream-ordered and does NOT wait for the stream.  No atomics anywhere.
 *
 * The ROI is three resident tables (BlockRoi.device_tables):
 *   row_keys   int64  [n_rows]      z * 2^32 + (y + 2^31) of every block row, ascending
 *   row_start  int32  [n_rows + 1]  CSR: the runs of row r are row_start[r] .. row_start[r + 1]
 *   runs_x     int32  [n_runs][2]   (x0, x1) in blocks, x1 inclusive, ascending and disjoint
 *                                   within a row
 * n_rows = 0 is the empty ROI (the pointers must still be valid).  The block of a voxel
 * coordinate v is floor(v / block_size), for negative v too.
 */
#ifndef FPLROI_H
#define FPLROI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLR_ABI_VERSION 1
#define FPLR_BLOCK 256
/* fplr_mask_box renders FPLR_BLOCK / 64 voxel rows per workgroup and launches at most this many
 * workgroups: a larger box is covered by a grid stride */
#define FPLR_MAX_GRID 4096
/* block_size lies in [1, 2^FPLR_BLOCK_SIZE_BITS]; the sides of a box in [1, 2^FPLR_SIDE_BITS);
 * an origin within +-2^FPLR_COORD_BITS */
#define FPLR_BLOCK_SIZE_BITS 20
#define FPLR_SIDE_BITS 21
#define FPLR_COORD_BITS 40

const char *fplr_last_error(void);
int fplr_abi_version(void);

/* out (device, uint8, dims[0]*dims[1]*dims[2], any alignment) = 1 where the voxel origin + (z, y,
 * x) lies in the ROI, else 0.  origin and dims are host arrays of (z, y, x).  A wave per voxel row:
 * the block row by binary search, then the row's runs; 16-byte stores at 16-byte aligned
 * addresses in the body, byte stores at the ragged ends.  Every byte of the box is written
 * exactly once and nothing outside it.  Refused: a box of 2^31 voxels or more.
 * replaces: libdvid's DVIDNodeService.get_roi3D */
int fplr_mask_box(const int64_t *row_keys, const int32_t *row_start, const int32_t *runs_x,
                  int64_t n_rows, int64_t n_runs, int32_t block_size, const int64_t origin[3],
                  const int64_t dims[3], uint8_t *out, void *stream);

/* flags[i] (device, uint8) = 1 when the point zyx[3 i .. 3 i + 2] (device, int64, (z, y, x)
 * voxels) lies in the ROI, else 0; n = 0 launches nothing.
 * replaces: libdvid's DVIDNodeService.roi_ptquery */
int fplr_ptquery(const int64_t *row_keys, const int32_t *row_start, const int32_t *runs_x,
                 int64_t n_rows, int64_t n_runs, int32_t block_size, const int64_t *zyx, int64_t n,
                 uint8_t *flags, void *stream);

/* counts[s] (device, int64) = the ROI voxels inside box s of `boxes` (device, int64, rows of
 * (z, y, x, dz, dy, dx)).  One workgroup per box; the threads' partial sums are added in a fixed
 * order in LDS; integers only, so the result does not depend on the launch geometry.  The boxes
 * are resident and cannot be checked here: a side outside [0, 2^FPLR_SIDE_BITS) or an origin
 * outside +-2^FPLR_COORD_BITS counts 0.  n_boxes = 0 launches nothing. */
int fplr_box_counts(const int64_t *row_keys, const int32_t *row_start, const int32_t *runs_x,
                    int64_t n_rows, int64_t n_runs, int32_t block_size, const int64_t *boxes,
                    int64_t n_boxes, int64_t *counts, void *stream);

/* out (device, f32, dims[0]*dims[1]*dims[2], 4-byte aligned) = (v - mean) / std, v the uint8 voxel
 * origin + (z, y, x) of vol (device, uint8, extent[0]*extent[1]*extent[2]) or 0 outside it: one
 * float32 subtraction and one correctly rounded float32 division, numpy's
 * (cube.astype('float32') - mean) / std.  16-byte stores at 16-byte aligned addresses, 4-byte
 * stores at the two ends of the buffer.  Refused: a box of 2^31 voxels or more.
 * replaces: get_gray3D and the normalisation of fplsynapses.roi_to_substacks */
int fplr_cut_normalize_u8(const uint8_t *vol, const int64_t extent[3], const int64_t origin[3],
                          const int64_t dims[3], float mean, float std, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FPLROI_H */
