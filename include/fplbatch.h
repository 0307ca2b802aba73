/* libfplbatch.so: training batches cut and augmented on the GPU (gfx950).
 *
 * A library of its own beside libfplhip.so (include/fplhip.h): no context object, raw
 * device pointers and a hipStream_t.  Every function but fplb_last_error returns 0 on
 * success and a non-zero rc with a thread-local message otherwise; no C++ exception
 * crosses this boundary.
 *
 * One call of fplb_gather is one kernel launch: per example of the batch it cuts a
 * (s0,s1,s2) patch around a centre of one of the resident volumes, applies
 * rot90(k, axes (1,2)) -> flip of axis 1 or 2 -> flip of axis 0, optionally the intensity
 * noise m * v + a, and writes float32 data and uint8 labels (the same transform on a 6^3
 * block around the centre, or the single centre voxel).  The host generators of
 * flypylib_amd/fplobjdetect.py are the specification; the output is bit-identical.
 */
#ifndef FPLBATCH_H
#define FPLBATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLB_ABI_VERSION 1

#define FPLB_U8 0
#define FPLB_F32 1

#define FPLB_LABELS_CENTRE 0 /* labels (B,1,1,1): the centre voxel, untransformed */
#define FPLB_LABELS_6 1      /* labels (B,6,6,6): transformed like the data        */

#define FPLB_FLIP_AXIS0 1u
#define FPLB_FLIP_AXIS1 2u
#define FPLB_FLIP_AXIS2 4u

/* one resident training volume (device memory, C order, dims d0 x d1 x d2) */
typedef struct fplb_volume {
  const void *image;     /* uint8 or float32 voxels (dtype)            */
  const uint8_t *labels; /* uint8 voxels, same dims                    */
  int32_t d0, d1, d2;
  int32_t dtype;         /* FPLB_U8 / FPLB_F32                         */
} fplb_volume;           /* 32 bytes */

/* one example of a batch */
typedef struct fplb_record {
  int32_t vol;     /* index into the volume table                                  */
  int32_t z, y, x; /* centre; the patch is [c - s/2, c + s/2) per axis             */
  uint8_t rot;     /* 0..3: np.rot90(v, rot, (1, 2)), applied first                 */
  uint8_t flips;   /* FPLB_FLIP_* bits, applied after the rotation                 */
  uint8_t pad_[6];
  double mul, add; /* intensity noise (used by the noise variants of the kernel)   */
} fplb_record;     /* 40 bytes */

const char *fplb_last_error(void);
int fplb_abi_version(void);
/* sizeof(fplb_volume), sizeof(fplb_record): the binding checks its numpy dtypes against them */
int fplb_struct_sizes(int32_t *volume_bytes, int32_t *record_bytes);

/* Cut one batch.  vols_dev[n_vols] and recs_dev[batch] are device memory; data_out is
 * batch*s0*s1*s2 float32, labels_out batch*216 or batch*1 uint8 (label_mode), both device
 * memory.  s0, s1, s2 are even; a record with an odd rot needs s1 == s2.  src_dtype is the
 * dtype of every volume the records name; noise != 0 applies
 *   float32 source: fl32(fl32(mul) * v) + fl32(add)         (no contraction)
 *   uint8 source:   fl32(mul * double(v) + add)             (double arithmetic, one rounding)
 * A record that names no volume, a volume of another dtype or a patch that does not lie
 * inside its volume writes nothing (the caller validates records; the kernel never reads
 * or writes out of bounds for them).  `stream` is a hipStream_t; the launch is asynchronous. */
int fplb_gather(const fplb_volume *vols_dev, int32_t n_vols, const fplb_record *recs_dev,
                int32_t batch, int32_t s0, int32_t s1, int32_t s2, int32_t src_dtype,
                int32_t noise, int32_t label_mode, float *data_out, uint8_t *labels_out,
                void *stream);

#ifdef __cplusplus
}
#endif
#endif
