/*
 * fplval.h - C ABI of libfplval.so: the loss and metric sums of a batch of predictions against
 * its labels, without a training step - what held-out validation (FplNetwork.evaluate, the val_
 * columns of FplNetwork.train) reduces after fpl_program_forward has run the inference-mode
 * network.  No gradient is written and no context of libfplhip.so is needed.
 *
 * Conventions of the side libraries: 0 on success, else non-zero with the text in
 * fplv_last_error() (thread-local); no C++ exception crosses the boundary; every argument is
 * checked before anything is launched.  `stream` is a hipStream_t (NULL: the default stream);
 * the call is stream-ordered and does NOT wait for the stream.
 *
 * The launch is fixed by n and pred's alignment alone (never by the device): FPLV_BLOCK threads
 * per block, each taking FPLV_ELEMS_PER_THREAD consecutive elements per grid stride, min(ceil(n
 * / (FPLV_BLOCK * FPLV_ELEMS_PER_THREAD)), FPLV_MAX_BLOCKS) blocks (the grid cap; at least one).
 * Every block writes its seven partial sums to `scratch`, a second launch of one block adds
 * them in block order: no float atomics, and the same input gives the same bits whatever the
 * scheduling.
 */
#ifndef FPLVAL_H
#define FPLVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPLV_ABI_VERSION 1
#define FPLV_BLOCK 256
#define FPLV_ELEMS_PER_THREAD 4
#define FPLV_MAX_BLOCKS 1024
#define FPLV_N_SUMS 8
/* FPLV_MAX_BLOCKS x 7 doubles */
#define FPLV_SCRATCH_BYTES 57344

/* the values of fpl_loss (fplhip.h) */
enum fplv_loss {
  FPLV_LOSS_BCE = 0,
  FPLV_LOSS_MASKED_BCE = 1,
  FPLV_LOSS_MASKED_WEIGHTED_BCE = 2,
  FPLV_LOSS_MASKED_FOCAL = 3
};

const char *fplv_last_error(void);
int fplv_abi_version(void);

/* sums[0..7] (device, doubles) of n predictions `pred` (device, f32, sigmoid outputs) against
 * `labels` (device, u8: 0, 1, or 2 = don't care), as fpl_trainer_metric_sums reports them for a
 * training batch:
 *   [0] the sum of the per-element loss `loss_kind` (clip at 1e-7, pos_weight 100, mask = y != 2,
 *       focal: y < 2), evaluated in DOUBLE from the float32 p
 *   [1] the count of rintf(p) == y              [2] of rintf(p * m) == y * m, m = y != 2
 *   [3] the sum of p over y == 0                [4] the count of y == 0
 *   [5] the sum of 1 - p (f32) over y == 1      [6] the count of y == 1
 *   [7] n
 * accumulate != 0: the eight values are ADDED to what `sums` holds (several batches, one
 * download); else they replace it.  `pred` and `labels` need no alignment beyond their element
 * size: elements before pred's first 16-byte boundary and the n % 4 remainder take a scalar
 * path.  `scratch` (device, 8-byte aligned, at least FPLV_SCRATCH_BYTES) is overwritten.
 * Refused before any launch: n < 1 or n > 2^31 - 1, an unknown loss_kind, a null pointer, a
 * scratch below FPLV_SCRATCH_BYTES, a misaligned pred, sums or scratch.
 * replaces: the evaluation pass of fit_generator(validation_data=...) (Keras' test_on_batch) */
int fplv_loss_sums(const float *pred, const uint8_t *labels, int64_t n, int32_t loss_kind,
                   int32_t accumulate, double *sums, void *scratch, int64_t scratch_bytes,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FPLVAL_H */
