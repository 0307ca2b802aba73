// libfplbatch.so (include/fplbatch.h): one kernel that cuts, rotates, flips and (for
// gen_volume2) adds intensity noise to a whole training batch from resident volumes.
//
// Layout.  A block of 256 threads (32 x 8) owns a 32 x 32 tile of one (j,k) plane of one
// example: grid = (s0 * tiles_j * tiles_k, batch).  The kernel indexes by OUTPUT voxel and
// derives the source voxel from the inverse of  rot90(k,(1,2)) -> flips:
//   * rot 0 / 2: an output row is a source row (possibly reversed).  The 32 lanes of a
//     half-wave read 32 consecutive source voxels and write 32 consecutive floats; no LDS.
//   * rot 1 / 3: an output row is a source column.  The block first copies the source
//     tile row-wise into LDS (lanes along the source's contiguous axis), then writes the
//     output tile row-wise reading LDS column-wise.  The tile is padded to 33 floats per
//     row: ds_read_b32 banks are (addr/4) mod 32 per 32-lane half, so a column read with
//     stride 33 touches 32 different banks.  Both global sides stay coalesced.
// The first block of every example also writes its labels (216 voxels or one).
//
// The arithmetic of the noise variants is spelled with __fmul_rn / __fadd_rn (and the
// double forms) so that no FMA contraction changes a last bit or the sign of a zero:
// the batches are bit-identical to the host generators'.
#include <hip/hip_runtime.h>

#include "fplbatch.h"
#include "../side/side_abi.h"

// this library's spelling of the shared shell
#define FPLB_EXPORT SIDE_EXPORT
#define FPLB_CATCH() SIDE_CATCH()
#define fplb_fail side_fail

namespace {

constexpr int TILE = 32;
constexpr int ROWS = 8;      // 256 threads = 32 lanes x 8 rows

// source (sj, sk) of output (j, k) in a plane of n1 x n2 outputs: flips undone first
// (they were applied last), then the rotation.  For an odd rot n1 == n2.
__device__ __forceinline__ void source_jk(int rot, unsigned flips, int n1, int n2, int j, int k,
                                          int &sj, int &sk) {
  if (flips & FPLB_FLIP_AXIS1) j = n1 - 1 - j;
  if (flips & FPLB_FLIP_AXIS2) k = n2 - 1 - k;
  switch (rot) {
    case 0: sj = j; sk = k; break;
    case 1: sj = k; sk = n1 - 1 - j; break;            // rot90(m)[j,k] = m[k, n-1-j]
    case 2: sj = n1 - 1 - j; sk = n2 - 1 - k; break;
    default: sj = n2 - 1 - k; sk = j; break;           // rot90(m,3)[j,k] = m[n-1-k, j]
  }
}

template <typename SrcT, bool NOISE>
__device__ __forceinline__ float to_out(SrcT v, double mul, double add);

template <> __device__ __forceinline__ float to_out<float, false>(float v, double, double) { return v; }
template <> __device__ __forceinline__ float to_out<uint8_t, false>(uint8_t v, double, double) {
  return (float)v;
}
template <> __device__ __forceinline__ float to_out<float, true>(float v, double mul, double add) {
  return __fadd_rn(__fmul_rn((float)mul, v), (float)add);
}
template <> __device__ __forceinline__ float to_out<uint8_t, true>(uint8_t v, double mul, double add) {
  return (float)__dadd_rn(__dmul_rn(mul, (double)v), add);
}

template <typename SrcT, bool NOISE>
__global__ __launch_bounds__(TILE * ROWS) void gather_kernel(
    const fplb_volume *__restrict__ vols, int n_vols, const fplb_record *__restrict__ recs,
    int s0, int s1, int s2, int tiles_k, int tiles_jk, int src_dtype, int label_mode,
    float *__restrict__ data, uint8_t *__restrict__ labels) {
  __shared__ float tile[TILE][TILE + 1];
  const int b = blockIdx.y;
  const fplb_record r = recs[b];
  // every test below is uniform over the block (one record per block)
  if ((unsigned)r.vol >= (unsigned)n_vols || r.rot > 3) return;
  const fplb_volume v = vols[r.vol];
  if (v.dtype != src_dtype) return;
  if ((r.rot & 1) && s1 != s2) return;
  const int o0 = r.z - s0 / 2, o1 = r.y - s1 / 2, o2 = r.x - s2 / 2;
  if (o0 < 0 || o1 < 0 || o2 < 0 || o0 + s0 > v.d0 || o1 + s1 > v.d1 || o2 + s2 > v.d2) return;
  const int lh = label_mode == FPLB_LABELS_6 ? 3 : 0;
  if (r.z - lh < 0 || r.y - lh < 0 || r.x - lh < 0 || r.z + lh > v.d0 || r.y + lh > v.d1 ||
      r.x + lh > v.d2 || r.z >= v.d0 || r.y >= v.d1 || r.x >= v.d2)
    return;
  const int rot = r.rot;
  const unsigned flips = r.flips;
  const long long d1 = v.d1, d2 = v.d2;
  const int tid = threadIdx.x;

  if (blockIdx.x == 0) {
    if (label_mode == FPLB_LABELS_6) {
      if (tid < 216) {
        int i = tid / 36, j = (tid / 6) % 6, k = tid % 6, sj, sk;
        if (flips & FPLB_FLIP_AXIS0) i = 5 - i;
        source_jk(rot, flips, 6, 6, j, k, sj, sk);
        labels[(long long)b * 216 + tid] =
            v.labels[((r.z - 3 + i) * d1 + (r.y - 3 + sj)) * d2 + (r.x - 3 + sk)];
      }
    } else if (tid == 0) {
      labels[b] = v.labels[(r.z * d1 + r.y) * d2 + r.x];
    }
  }

  const int i = blockIdx.x / tiles_jk;
  const int t = blockIdx.x % tiles_jk;
  const int j0 = (t / tiles_k) * TILE, k0 = (t % tiles_k) * TILE;
  const int tw_j = min(TILE, s1 - j0), tw_k = min(TILE, s2 - k0);
  const int si = (flips & FPLB_FLIP_AXIS0) ? s0 - 1 - i : i;
  const int tx = tid & (TILE - 1), ty = tid / TILE;
  const SrcT *plane = (const SrcT *)v.image + ((o0 + si) * d1 + o1) * d2 + o2;
  float *out = data + (((long long)b * s0 + i) * s1 + j0) * s2 + k0;

  if (!(rot & 1)) {
    if (tx < tw_k)
      for (int jj = ty; jj < tw_j; jj += ROWS) {
        int sj, sk;
        source_jk(rot, flips, s1, s2, j0 + jj, k0 + tx, sj, sk);
        out[(long long)jj * s2 + tx] = to_out<SrcT, NOISE>(plane[sj * d2 + sk], r.mul, r.add);
      }
    return;
  }
  // transposed: sj depends on k only and sk on j only; the tile's source rectangle is
  // [sj_lo, sj_lo + tw_k) x [sk_lo, sk_lo + tw_j)
  int sja, ska, sjb, skb;
  source_jk(rot, flips, s1, s2, j0, k0, sja, ska);
  source_jk(rot, flips, s1, s2, j0 + tw_j - 1, k0 + tw_k - 1, sjb, skb);
  const int sj_lo = min(sja, sjb), sk_lo = min(ska, skb);
  if (tx < tw_j)
    for (int a = ty; a < tw_k; a += ROWS)
      tile[a][tx] = to_out<SrcT, NOISE>(plane[(sj_lo + a) * d2 + (sk_lo + tx)], r.mul, r.add);
  __syncthreads();
  if (tx < tw_k)
    for (int jj = ty; jj < tw_j; jj += ROWS) {
      int sj, sk;
      source_jk(rot, flips, s1, s2, j0 + jj, k0 + tx, sj, sk);
      out[(long long)jj * s2 + tx] = tile[sj - sj_lo][sk - sk_lo];
    }
}

template <typename SrcT, bool NOISE>
int launch(const fplb_volume *vols, int n_vols, const fplb_record *recs, int batch, int s0, int s1,
           int s2, int src_dtype, int label_mode, float *data, uint8_t *labels, hipStream_t st) {
  const int tiles_j = (s1 + TILE - 1) / TILE, tiles_k = (s2 + TILE - 1) / TILE;
  dim3 grid((unsigned)(s0 * tiles_j * tiles_k), (unsigned)batch);
  hipLaunchKernelGGL((gather_kernel<SrcT, NOISE>), grid, dim3(TILE * ROWS), 0, st, vols, n_vols,
                     recs, s0, s1, s2, tiles_k, tiles_j * tiles_k, src_dtype, label_mode, data,
                     labels);
  return launched("fplb_gather");
}

}  // namespace

FPLB_EXPORT const char *fplb_last_error(void) try {
  return side_err;
} catch (...) { return "fplb_last_error: C++ exception"; }

FPLB_EXPORT int fplb_abi_version(void) try {
  return FPLB_ABI_VERSION;
} FPLB_CATCH()

FPLB_EXPORT int fplb_struct_sizes(int32_t *volume_bytes, int32_t *record_bytes) try {
  if (!volume_bytes || !record_bytes) return fplb_fail("fplb_struct_sizes: null argument");
  *volume_bytes = (int32_t)sizeof(fplb_volume);
  *record_bytes = (int32_t)sizeof(fplb_record);
  return 0;
} FPLB_CATCH()

FPLB_EXPORT int fplb_gather(const fplb_volume *vols_dev, int32_t n_vols,
                            const fplb_record *recs_dev, int32_t batch, int32_t s0, int32_t s1,
                            int32_t s2, int32_t src_dtype, int32_t noise, int32_t label_mode,
                            float *data_out, uint8_t *labels_out, void *stream) try {
  if (!vols_dev || !recs_dev || !data_out || !labels_out)
    return fplb_fail("fplb_gather: null pointer argument");
  if (n_vols < 1 || batch < 1 || batch > 65535)
    return fplb_fail("fplb_gather: n_vols %d, batch %d (1..65535)", n_vols, batch);
  if (s0 < 2 || s1 < 2 || s2 < 2 || (s0 | s1 | s2) & 1 || s0 > 4096 || s1 > 4096 || s2 > 4096)
    return fplb_fail("fplb_gather: context (%d,%d,%d) must be even, 2..4096 per axis", s0, s1, s2);
  if (label_mode != FPLB_LABELS_CENTRE && label_mode != FPLB_LABELS_6)
    return fplb_fail("fplb_gather: label_mode %d", label_mode);
  hipStream_t st = (hipStream_t)stream;
#define FPLB_GO(T, N) \
  return launch<T, N>(vols_dev, n_vols, recs_dev, batch, s0, s1, s2, src_dtype, label_mode, \
                      data_out, labels_out, st)
  if (src_dtype == FPLB_F32) {
    if (noise) FPLB_GO(float, true);
    FPLB_GO(float, false);
  }
  if (src_dtype == FPLB_U8) {
    if (noise) FPLB_GO(uint8_t, true);
    FPLB_GO(uint8_t, false);
  }
#undef FPLB_GO
  return fplb_fail("fplb_gather: src_dtype %d (FPLB_U8 or FPLB_F32)", src_dtype);
} FPLB_CATCH()
