/*
 * fplseg.h - C ABI of libfplseg.so: reads of a label volume RESIDENT in device memory that need
 * no context of libfplhip.so - the labels of a point list, and the padded u64 copy of a box
 * that fpl_v2o_set_seg (FPL_MEM_DEVICE_BOX, fplhip.h) makes inside a context, here into a
 * caller's buffer with the same kernel (csrc/seg_box.h), which is how the tests hold that
 * kernel to numpy element by element.
 *
 * Conventions of the side libraries: 0 on success, else non-zero with the text in
 * fpls_last_error() (thread-local); no C++ exception crosses the boundary.  Volumes are
 * (Z,Y,X), X fastest, contiguous, 4 or 8 bytes per label (`seg_bytes`); labels are widened to
 * u64.  Extents, dims and origins lie in the 2^21 coordinate range of fpl_crop_substack_u8.
 * `stream` is a hipStream_t (NULL: the default stream); both calls return after it has drained.
 */
#ifndef FPLSEG_H
#define FPLSEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLS_ABI_VERSION 1
enum fpls_mem { FPLS_MEM_HOST = 0, FPLS_MEM_DEVICE = 1 };

const char *fpls_last_error(void);
int fpls_abi_version(void);

/* dst (device, u64, (dims + 2r) voxels) := the box origin .. origin + dims of `vol` (device,
 * extents `extent`) in a zero shell of r; zeros where the box leaves the volume, all zeros
 * where it misses it.  `vol` and `dst` must be device memory. */
int fpls_pad_box(const void *vol, int32_t seg_bytes, const int64_t extent[3],
                 const int64_t origin[3], const int64_t dims[3], int32_t r, uint64_t *dst,
                 void *stream);

/* out[i] = vol[zyx[i]] for n (z, y, x) int64 triples; `zyx` and `out` (n u64) are each in host
 * or device memory (fpls_mem).  A triple outside the volume is an error: host triples are
 * checked before anything is launched, and the kernel checks every triple, reads nothing for
 * one outside and raises a flag.  A failed call leaves `out` as it was.  n == 0 returns at
 * once.  replaces: the numpy indexing of a host label array by _get_labels
 * (fplobjdetect.py:457-461) */
int fpls_gather_labels(const void *vol, int32_t seg_bytes, const int64_t extent[3],
                       const int64_t *zyx, int zyx_mem, int64_t n, uint64_t *out, int out_mem,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FPLSEG_H */
