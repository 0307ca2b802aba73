// Op plan of the fp32 MFMA executor (conv_mfma_f32.hip): which programs it runs, the kernel launch
// groups of one forward in order, the operands of each as symbolic views, the template instance
// each launch takes and where each op's weight fragments lie in the program's fragment buffer.
// fpl_mfma_f32_supported is this plan's `ok`; the packing pass and the launch loop walk its steps
// and hold no copy of the limits, of the fusion rule or of a fragment size.  Plain C++ on standard
// headers and the public fplhip.h (fpl_op and the enums): a host compiler builds it alone
// (tests/test_mfma_f32_plan_host.py does, and prints the plan of every test program).  It reads
// no environment: the caller passes FPL_F32_UNFUSED in.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/fplhip.h"

namespace f32plan {

// ---- the kernel instances conv_mfma_f32.hip compiles: every width limit, once ---------------
// conv3_f32<1..4>, atrous3_f32<1..4>, stem_cin1_f32<1..4>: up to 4 blocks of 16 outputs a launch;
// a wider 3x3x3 (plain or dilated) runs in slices of 64 outputs, a wider stem does not exist
constexpr int MB_MAX = 4;
constexpr int SLICE = 16 * MB_MAX;
constexpr int CONV3_COUT_MAX = 256;
constexpr int SLICES_MAX = CONV3_COUT_MAX / SLICE;
constexpr int CONV3_CHUNKS_MAX = 12;          // Conv3F::src[12]: 16-channel chunks of the input
constexpr int CONV1_MB[] = {1, 2, 3, 4, 6, 8};  // conv1_f32<1, 2, 3, 4, 6, 8>
constexpr int FUSED_MB[] = {2, 3, 4};         // conv3_f32<MB, MB, POOL>: conv3 + conv1 (+ pool)
constexpr int STEM_FUSED_MB[] = {2, 3};       // stem_conv1_pool_f32<MB, MB>: the pooled form only
constexpr int GEMM2_C_MAX = 256;              // deconv2_f32 / down2_f32: channels in and out

template <size_t N>
inline bool among(const int (&table)[N], int v) {
  for (int t : table)
    if (t == v) return true;
  return false;
}
inline int blocks16(int c) { return (c + 15) / 16; }

// ---- fragment sizes in floats: the pack_*_f32 functions size their output from these --------
inline size_t conv3_frag_floats(int cin, int mb) { return (size_t)blocks16(cin) * 27 * mb * 256; }
inline size_t conv1_frag_floats(int cin, int mb) { return (size_t)blocks16(cin) * mb * 256; }
inline size_t stem_frag_floats(int mb) { return (size_t)2 * mb * 256; }
// Conv3DTranspose: N = 2 cout columns per (a, b) tap row in nb2 blocks; the shifts follow
inline int deconv_nb2(int cout) { return blocks16(2 * cout); }
inline size_t deconv_shift_off(int cin, int cout) { return (size_t)4 * deconv_nb2(cout) * blocks16(cin) * 256; }
inline size_t deconv_frag_floats(int cin, int cout) { return deconv_shift_off(cin, cout) + (size_t)16 * deconv_nb2(cout); }
// the instance of down2_f32 that runs cin -> cout: K-blocks per tap pair held in registers
// (0: the any-cin form) and the N-blocks per pass, which the fragments are padded to
inline void down_form(int cin, int *nkb_reg, int *nbt) {
  const int nkb = blocks16(2 * cin);
  *nkb_reg = nkb <= 2 ? nkb : 0;
  *nbt = nkb <= 2 ? 2 : 4;
}
inline int down_nbp(int cin, int cout) {
  int nkb_reg, nbt;
  down_form(cin, &nkb_reg, &nbt);
  return (blocks16(cout) + nbt - 1) / nbt * nbt;
}
inline size_t down_shift_off(int cin, int cout) { return (size_t)4 * blocks16(2 * cin) * down_nbp(cin, cout) * 256; }
inline size_t down_frag_floats(int cin, int cout) { return down_shift_off(cin, cout) + (size_t)16 * down_nbp(cin, cout); }

// ---- the plan ------------------------------------------------------------------------------
enum Form {
  STEM, STEM_CONV1_POOL, CONV3, CONV3_CONV1, CONV3_CONV1_POOL, CONV1, ATROUS, DECONV, DOWN, POOL, ADD, CONCAT,
  N_FORMS
};
inline const char *form_name(int f) {
  static const char *const names[N_FORMS] = {"stem", "stem_conv1_pool", "conv3", "conv3_conv1", "conv3_conv1_pool",
                                             "conv1", "atrous", "deconv", "down", "pool", "add", "concat"};
  return f >= 0 && f < N_FORMS ? names[f] : "?";
}

// a materialised tensor seen through an UpSampling3D or a Cropping3D (up = 1, crop = 0: as it is)
struct View {
  int tensor = -1, up = 1, crop = 0;
};
// 64 outputs [c0, c0 + cs) of a plain or dilated 3x3x3, mb blocks of 16, fragments at frag_off
struct Slice {
  int c0 = 0, cs = 0, mb = 0;
  size_t frag_off = 0;
};
// one kernel launch group
struct Step {
  int form = N_FORMS;
  int op[3] = {-1, -1, -1};     // the op, then the 1x1x1 conv and the pool fused into its kernel
  int n_ops = 0;
  int dst = -1;                 // tensor the step writes: the last op's
  View src[2];                  // conv3: the chunks' sources in order (two: through a concatenation);
  int n_src = 0;                // add, concat: both operands
  int mb = 0, mb1 = 0;          // blocks of 16 outputs of the kernel's instance (mb1: the fused conv1's)
  bool pool = false;
  Slice slice[SLICES_MAX];      // conv3 forms and atrous (a fused conv3 is one slice)
  int n_slices = 0;
  // the step's fragments, [frag_off, frag_off + frag_len) of the program's buffer, in floats: the
  // slices back to back, or one block with the shifts at frag_off + shift_off (deconv, down), then
  // the fused conv1's at frag1_off
  size_t frag_off = 0, frag_len = 0, shift_off = 0, frag1_off = 0;
};
struct Plan {
  bool ok = true;
  int bad_op = -1;              // !ok: the first op the executor cannot run, and why
  const char *reason = "";
  // every op is a voxel GEMM (1x1x1 conv, Conv3DTranspose, strided Conv3D(2)) or a dilated Conv3D,
  // whose kernel takes three extents: the program runs on tiles of any extents.  The rest is
  // written for cubic tiles
  bool any_dims = true;
  bool has_gemm2_or_dilated = false;   // ... and holds one that is no 1x1x1 conv
  std::vector<Step> steps;
  size_t frag_floats = 0;
  // the dispatchers' question.  (A program of 1x1x1 convs alone on tiles that are not cubic
  // stays with the per-op executor, as it always has.)
  bool takes(bool cubic) const { return ok && (cubic || (any_dims && has_gemm2_or_dilated)); }
};

// Lowers a program.  It runs on this executor when
//  * every tensor is written once and read after that, channel counts agree (fpl_infer_shapes
//    refuses the others for every executor), and the output is a materialised tensor;
//  * up / crop views are views of materialised tensors, and views and virtual concatenations are
//    read by multi-channel 3x3x3 convs only - but an add may read crops, and a concatenation that
//    is written out may read views;
//  * a concatenation stays virtual (two views, resolved by the conv3 that loads it) in every
//    program of the kinds the executor has always run.  In a program that holds a Conv3DTranspose
//    one whose readers are not all multi-channel conv3s is written out instead, so that a 1x1x1
//    conv may read it.  Either way the conv3 reads the two operands, which are no concatenations,
//    and the second starts on a 16-channel chunk;
//  * the widths are those of the instances above; pools of 2, ups of 1 or 2, crops equal on all
//    six faces.
// conv3 -> conv1 (-> pool2) run as ONE kernel when the intermediate tensors have no other reader:
// the 1x1x1 conv is chained in registers, the pool is an epilogue (`unfused`: one kernel per op,
// for A/B runs).  The fragments do not depend on `unfused`.
inline Plan plan(const fpl_op *ops, size_t n_ops, int n_tensors, int out_tensor, bool unfused) {
  Plan P;
  auto fail = [&P](size_t i, const char *why) -> Plan & {
    P.ok = false; P.bad_op = (int)i; P.reason = why;
    P.steps.clear(); P.frag_floats = 0;
    return P;
  };
  for (size_t i = 0; i < n_ops; ++i) {
    const bool gemm2 = ops[i].kind == FPL_OP_DECONV || ops[i].kind == FPL_OP_DOWN || ops[i].kind == FPL_OP_DILATED;
    P.has_gemm2_or_dilated |= gemm2;
    P.any_dims &= gemm2 || (ops[i].kind == FPL_OP_CONV && ops[i].k == 1);
  }
  if (n_tensors < 1 || out_tensor < 0 || out_tensor >= n_tensors) return fail(0, "tensor ids out of range");
  auto conv3m = [](const fpl_op &o) { return o.kind == FPL_OP_CONV && o.k == 3 && o.cin > 1; };
  // per tensor: its readers (the program's output counts as one), and whether one of them is
  // no multi-channel conv3
  std::vector<int> readers(n_tensors, 0);
  std::vector<char> other_reader(n_tensors, 0);
  readers[out_tensor] = 1; other_reader[out_tensor] = 1;
  bool has_deconv = false;
  for (size_t i = 0; i < n_ops; ++i) {
    const fpl_op &op = ops[i];
    if (op.src0 < 0 || op.src0 >= n_tensors || op.src1 >= n_tensors || op.dst <= 0 || op.dst >= n_tensors)
      return fail(i, "tensor ids out of range");
    has_deconv |= op.kind == FPL_OP_DECONV;
    ++readers[op.src0];
    if (op.src1 >= 0) ++readers[op.src1];
    if (conv3m(op)) continue;
    other_reader[op.src0] = 1;
    if (op.src1 >= 0) other_reader[op.src1] = 1;
  }
  // what a tensor is while the ops are walked
  enum Kind { NONE, BUFFER, VIEW, CAT };       // CAT: a virtual concatenation
  struct Sym {
    Kind kind = NONE;
    View v;
    int C = 0;
    int cat_op = -1;                           // the concatenation that made it, written out or not
  };
  std::vector<Sym> sym(n_tensors);
  std::vector<char> fused(n_ops, 0);           // the op runs inside an earlier step's kernel
  sym[0].kind = BUFFER; sym[0].v.tensor = 0; sym[0].C = 1;
  auto relu_or_none = [](const fpl_op &o) { return o.act == FPL_ACT_RELU || o.act == FPL_ACT_NONE; };
  auto pool2 = [](const fpl_op &o) { return o.kind == FPL_OP_POOL && o.p[0] == 2 && o.p[1] == 2 && o.p[2] == 2; };
  for (size_t i = 0; i < n_ops; ++i) {
    const fpl_op &op = ops[i];
    const bool binary = op.kind == FPL_OP_CONCAT || op.kind == FPL_OP_ADD;
    if (sym[op.src0].kind == NONE || (binary && (op.src1 < 0 || sym[op.src1].kind == NONE)))
      return fail(i, "reads a tensor before it is produced");
    if (sym[op.dst].kind != NONE) return fail(i, "writes a tensor twice");
    const Sym a = sym[op.src0], b = op.src1 >= 0 ? sym[op.src1] : Sym();
    const bool v0 = a.kind != BUFFER, v1 = b.kind == VIEW || b.kind == CAT;
    Sym o;
    o.kind = BUFFER; o.v.tensor = op.dst; o.C = a.C;
    Step s;
    s.op[0] = (int)i; s.n_ops = 1; s.dst = op.dst;
    s.src[0] = a.v; s.n_src = 1;
    s.frag_off = P.frag_floats;
    bool launches = true;
    switch (op.kind) {
      case FPL_OP_UP:
        if (op.p[0] != op.p[1] || op.p[1] != op.p[2] || (op.p[0] != 1 && op.p[0] != 2))
          return fail(i, "an up-sampling that is not 1 or 2 on every axis");
        if (v0) return fail(i, "nested views");
        o.kind = VIEW; o.v = a.v; o.v.up = op.p[0];
        launches = false;
        break;
      case FPL_OP_CROP:
        for (int q = 1; q < 6; ++q)
          if (op.p[q] != op.p[0]) return fail(i, "a crop that is not equal on all six faces");
        if (op.p[0] < 0) return fail(i, "a negative crop");
        if (v0) return fail(i, "nested views");
        o.kind = VIEW; o.v = a.v; o.v.crop = op.p[0];
        launches = false;
        break;
      case FPL_OP_CONCAT:
        o.C = a.C + b.C; o.cat_op = (int)i;
        if (has_deconv && other_reader[op.dst]) {
          // written out - operands: buffers or up / crop views of buffers
          if (a.kind == CAT || b.kind == CAT) return fail(i, "concatenate of a concatenation");
          s.form = CONCAT; s.src[1] = b.v; s.n_src = 2;
        } else {
          o.kind = CAT; o.v = View();
          launches = false;
        }
        break;
      case FPL_OP_ADD:
        // operands may be cropped
        if (a.kind == CAT || b.kind == CAT || a.v.up != 1 || b.v.up != 1 || a.C != b.C)
          return fail(i, "add of incompatible tensors");
        s.form = ADD; s.src[1] = b.v; s.n_src = 2;
        break;
      case FPL_OP_POOL:
        if (!pool2(op)) return fail(i, "a pool that is not 2 x 2 x 2");
        if (v0 || v1) return fail(i, "pool of a view");
        s.form = POOL;
        break;
      case FPL_OP_DECONV:
      case FPL_OP_DOWN:
        if (op.k != 2 || op.cin < 1 || op.cout < 1 || op.cin > GEMM2_C_MAX || op.cout > GEMM2_C_MAX)
          return fail(i, "2x2x2 deconv / down: no kernel of this width");
        if (v0 || v1) return fail(i, op.kind == FPL_OP_DECONV ? "Conv3DTranspose of a view" : "strided Conv3D of a view");
        if (a.C != op.cin) return fail(i, "input channels are not the op's cin");
        o.C = op.cout;
        if (op.kind == FPL_OP_DECONV) {
          s.form = DECONV; s.shift_off = deconv_shift_off(op.cin, op.cout); s.frag_len = deconv_frag_floats(op.cin, op.cout);
        } else {
          s.form = DOWN; s.shift_off = down_shift_off(op.cin, op.cout); s.frag_len = down_frag_floats(op.cin, op.cout);
        }
        break;
      case FPL_OP_DILATED:
      case FPL_OP_CONV: {
        if (op.cin < 1 || op.cout < 1) return fail(i, "a convolution without channels");
        o.C = op.cout;
        s.mb = blocks16(op.cout);
        if (op.kind == FPL_OP_CONV && op.k == 1) {
          if (!among(CONV1_MB, s.mb)) return fail(i, "1x1x1 conv: no kernel of this width");
          if (v0 || v1) return fail(i, "conv1 of a view");
          if (a.C != op.cin) return fail(i, "input channels are not the op's cin");
          s.form = CONV1; s.frag_len = conv1_frag_floats(op.cin, s.mb);
          break;
        }
        if (op.k != 3) return fail(i, "a convolution that is not 1x1x1 or 3x3x3");
        const bool dilated = op.kind == FPL_OP_DILATED, stem = !dilated && op.cin == 1;
        if (stem) {
          if (s.mb > MB_MAX) return fail(i, "3x3x3 conv of one channel: no kernel of this width");
          if (v0 || v1) return fail(i, "stem of a view");
          if (a.C != 1) return fail(i, "input channels are not the op's cin");
          s.form = STEM; s.frag_len = stem_frag_floats(s.mb);
        } else {
          if (op.cout > CONV3_COUT_MAX || op.cin > 16 * CONV3_CHUNKS_MAX) return fail(i, "3x3x3 conv: no kernel of this width");
          int C = a.C;
          if (dilated) {
            if (v0 || v1) return fail(i, "dilated Conv3D of a view");
          } else {
            if (v1) return fail(i, "conv3 with a view as second operand");
            if (a.cat_op >= 0) {
              // a concatenation is read through its two operands, written out or not: channel
              // chunks of the concatenated tensor in order, each source on a 16-channel boundary
              const Sym va = sym[ops[a.cat_op].src0], vb = sym[ops[a.cat_op].src1];
              if (va.kind == CAT || vb.kind == CAT || va.C % 16 != 0) return fail(i, "unsupported concat");
              s.src[0] = va.v; s.src[1] = vb.v; s.n_src = 2;
              C = va.C + vb.C;
            }
          }
          if (C != op.cin) return fail(i, "input channels are not the op's cin");
          s.form = dilated ? ATROUS : CONV3;
          for (int c0 = 0; c0 < op.cout; c0 += SLICE) {
            Slice &sl = s.slice[s.n_slices++];
            sl.c0 = c0; sl.cs = op.cout - c0 < SLICE ? op.cout - c0 : SLICE; sl.mb = blocks16(sl.cs);
            sl.frag_off = s.frag_off + s.frag_len;
            s.frag_len += conv3_frag_floats(op.cin, sl.mb);
          }
        }
        if (dilated || unfused || i + 1 >= n_ops) break;
        // the fusion rule.  The Cin = 1 kernel exists only in its pooled form
        const fpl_op &n1 = ops[i + 1];
        if (!(n1.kind == FPL_OP_CONV && n1.k == 1 && n1.src0 == op.dst && readers[op.dst] == 1 &&
              blocks16(n1.cout) == s.mb && op.cout % 4 == 0 && relu_or_none(op)))
          break;
        const bool pl = i + 2 < n_ops && pool2(ops[i + 2]) && ops[i + 2].src0 == n1.dst && readers[n1.dst] == 1 &&
                        relu_or_none(n1);
        if (stem ? !(pl && among(STEM_FUSED_MB, s.mb)) : !among(FUSED_MB, s.mb)) break;
        s.form = stem ? STEM_CONV1_POOL : (pl ? CONV3_CONV1_POOL : CONV3_CONV1);
        s.mb1 = s.mb; s.pool = pl;
        s.op[1] = (int)i + 1; fused[i + 1] = 1;
        if (pl) { s.op[2] = (int)i + 2; fused[i + 2] = 1; }
        s.n_ops = pl ? 3 : 2;
        s.dst = ops[s.op[s.n_ops - 1]].dst;
        s.frag1_off = s.frag_off + s.frag_len;
        s.frag_len += conv1_frag_floats(n1.cin, s.mb1);
        break;
      }
      default:
        return fail(i, "an op kind the executor lacks");
    }
    sym[op.dst] = o;
    if (op.dst == out_tensor && o.kind != BUFFER) return fail(i, "the output is a view");
    if (fused[i] || !launches) continue;      // (a fused op was checked as any other; its fragments are its step's)
    P.frag_floats += s.frag_len;
    P.steps.push_back(s);
  }
  if (sym[out_tensor].kind != BUFFER) return fail(n_ops, "the output is never produced");
  return P;
}

}  // namespace f32plan
