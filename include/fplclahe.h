/*
 * fplclahe.h - C ABI of libfplclahe.so: per-slice contrast-limited adaptive histogram
 * equalisation (CLAHE) of a (Z, Y, X) volume resident on the GPU, what the reference's
 * fplutils.clahe does with skimage in a Python loop over z.  The specification is the package's
 * own (flypylib_amd/clahe.py: clahe_numpy), and the kernels reproduce it bit for bit; parity
 * with scikit-image is unpinned.
 *
 * Conventions of the side libraries: 0 on success, else non-zero with the text in
 * fplc_last_error() (thread-local); no C++ exception crosses the boundary; every argument is
 * checked before anything is launched.  `stream` is a hipStream_t (NULL: the default stream);
 * the call is stream-ordered and does NOT wait for the stream.
 *
 * Four stages, each one or two launches; the scratch carries the state from one to the next:
 *   FPLC_STAGE_RANGE   the raw min and max of every slice (integer atomics on order-preserving
 *                      keys: exact in any order), then the volume's mn and mx
 *   FPLC_STAGE_MAPS    one workgroup per tile (z, i, j): histogram in LDS (integer atomics), the
 *                      clip and its redistribution by one wave in the specification's order, an
 *                      inclusive scan, the uint16 map
 *   FPLC_STAGE_APPLY   one thread per pixel: the bilinear interpolation between four maps in
 *                      float64 without contraction, uint16 to scratch; the slice's min and max of
 *                      those by one integer atomic per wave
 *   FPLC_STAGE_FINISH  the rescale to float32 [0, 1], and zero_mean
 * No float atomics anywhere: equal input gives equal bits whatever the scheduling.
 */
#ifndef FPLCLAHE_H
#define FPLCLAHE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLC_ABI_VERSION 1
#define FPLC_BLOCK 256
#define FPLC_MAX_NBINS 256
#define FPLC_NR_OF_GRAY 16384
/* the head of the scratch: float mn, float mx, uint32 non-finite flag, one spare word */
#define FPLC_STATUS_BYTES 16

#define FPLC_STAGE_RANGE 1
#define FPLC_STAGE_MAPS 2
#define FPLC_STAGE_APPLY 4
#define FPLC_STAGE_FINISH 8
#define FPLC_STAGE_ALL 15

enum fplc_dtype { FPLC_U8 = 0, FPLC_F32 = 1 };

const char *fplc_last_error(void);
int fplc_abi_version(void);

/* *bytes = the scratch a call with these sizes needs (FPLC_STATUS_BYTES, 16 bytes per slice, the
 * uint16 maps of every tile, the uint16 interpolated volume; each part 16-byte aligned); sizes
 * fplc_clahe would refuse are refused here */
int fplc_scratch_bytes(int64_t Z, int64_t Y, int64_t X, int64_t ky, int64_t kx, int32_t nbins,
                       int64_t *bytes);

/* out (device, f32, Z*Y*X, 4-byte aligned) = CLAHE of `in` (device, Z*Y*X elements of `dtype`:
 * FPLC_U8 with any alignment, FPLC_F32 4-byte aligned), tiles of ky x kx pixels, histograms of
 * `nbins` bins clipped at `clim` counts (the caller's max(int(clip_limit ky kx), 1), or
 * FPLC_NR_OF_GRAY for no clipping), zero_mean != 0: 0.5 subtracted.  `stages`: the stages to
 * launch, in order (FPLC_STAGE_ALL for the function; a subset only to time a stage alone on a
 * scratch the earlier stages have filled).  `scratch` (device, 16-byte aligned, at least
 * fplc_scratch_bytes) is overwritten; after the range stage its first FPLC_STATUS_BYTES hold the
 * volume's mn and mx (f32) and a flag that is non-zero when a value is not finite.  A slice that
 * is constant, and every slice of a volume that is constant or holds non-finite values, comes
 * out 0.0 (- 0.5 with zero_mean); the caller reads the status to refuse such a volume.
 * Refused before any launch: a size below 1, Z*Y*X or ky*kx above 2^31 - 1, nbins outside
 * 2..FPLC_MAX_NBINS, clim below 1, an unknown dtype or stage, a null or misaligned pointer, a
 * scratch below fplc_scratch_bytes, memory that is not the device's.
 * replaces: fplutils.clahe's loop over skimage.exposure.equalize_adapthist */
int fplc_clahe(const void *in, int32_t dtype, int64_t Z, int64_t Y, int64_t X, int64_t ky,
               int64_t kx, int64_t clim, int32_t nbins, int32_t zero_mean, float *out,
               void *scratch, int64_t scratch_bytes, int32_t stages, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FPLCLAHE_H */
