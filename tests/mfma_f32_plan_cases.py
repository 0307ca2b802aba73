"""csrc/mfma_f32_plan.h asked through a small driver built with the host compiler, and the seeded
sweep of random small programs it is held to (tests/test_mfma_f32_plan_host.py).  Nothing here
touches a GPU."""
import json
import os
import shutil
import subprocess

import numpy as np

from flypylib_amd.program import (OP_ADD, OP_CONCAT, OP_CONV, OP_CROP, OP_DECONV, OP_DILATED, OP_DOWN, OP_POOL,
                                  OP_UP)
from tests.v2o_cases import host_cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stdin: one program per line - unfused n_tensors out_tensor n_ops, then per op
# kind src0 src1 dst k cin cout act p0..p5.  stdout: the header's constants, then one JSON plan per line
DRIVER = r'''
#include <cstdio>
#include <vector>
#include "mfma_f32_plan.h"
using namespace f32plan;
int main() {
  std::printf("{\"MB_MAX\":%d,\"SLICE\":%d,\"CONV3_COUT_MAX\":%d,\"SLICES_MAX\":%d,\"CONV3_CHUNKS_MAX\":%d,"
              "\"GEMM2_C_MAX\":%d,\"CONV1_MB\":[", MB_MAX, SLICE, CONV3_COUT_MAX, SLICES_MAX, CONV3_CHUNKS_MAX, GEMM2_C_MAX);
  for (size_t i = 0; i < sizeof(CONV1_MB) / sizeof(int); ++i) std::printf("%s%d", i ? "," : "", CONV1_MB[i]);
  std::printf("],\"FUSED_MB\":[");
  for (size_t i = 0; i < sizeof(FUSED_MB) / sizeof(int); ++i) std::printf("%s%d", i ? "," : "", FUSED_MB[i]);
  std::printf("],\"STEM_FUSED_MB\":[");
  for (size_t i = 0; i < sizeof(STEM_FUSED_MB) / sizeof(int); ++i) std::printf("%s%d", i ? "," : "", STEM_FUSED_MB[i]);
  std::printf("]}\n");
  int unfused, n_tensors, out_tensor, n_ops;
  while (std::scanf("%d %d %d %d", &unfused, &n_tensors, &out_tensor, &n_ops) == 4) {
    std::vector<fpl_op> ops(n_ops);
    for (fpl_op &o : ops) {
      o = fpl_op();
      if (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &o.kind, &o.src0, &o.src1, &o.dst, &o.k, &o.cin,
                     &o.cout, &o.act, &o.p[0], &o.p[1], &o.p[2], &o.p[3], &o.p[4], &o.p[5]) != 14)
        return 2;
    }
    const Plan p = plan(ops.data(), ops.size(), n_tensors, out_tensor, unfused != 0);
    std::printf("{\"ok\":%d,\"bad_op\":%d,\"reason\":\"%s\",\"any_dims\":%d,\"takes_cubic\":%d,\"takes_other\":%d,"
                "\"frag_floats\":%zu,\"steps\":[", (int)p.ok, p.bad_op, p.reason, (int)p.any_dims, (int)p.takes(true),
                (int)p.takes(false), p.frag_floats);
    for (size_t i = 0; i < p.steps.size(); ++i) {
      const Step &s = p.steps[i];
      std::printf("%s{\"form\":\"%s\",\"ops\":[", i ? "," : "", form_name(s.form));
      for (int q = 0; q < s.n_ops; ++q) std::printf("%s%d", q ? "," : "", s.op[q]);
      std::printf("],\"dst\":%d,\"src\":[", s.dst);
      for (int q = 0; q < s.n_src; ++q)
        std::printf("%s[%d,%d,%d]", q ? "," : "", s.src[q].tensor, s.src[q].up, s.src[q].crop);
      std::printf("],\"mb\":%d,\"mb1\":%d,\"pool\":%d,\"slices\":[", s.mb, s.mb1, (int)s.pool);
      for (int q = 0; q < s.n_slices; ++q)
        std::printf("%s[%d,%d,%d,%zu]", q ? "," : "", s.slice[q].c0, s.slice[q].cs, s.slice[q].mb, s.slice[q].frag_off);
      std::printf("],\"frag_off\":%zu,\"frag_len\":%zu,\"shift_off\":%zu,\"frag1_off\":%zu}", s.frag_off, s.frag_len,
                  s.shift_off, s.frag1_off);
    }
    std::printf("]}\n");
  }
  return 0;
}
'''

# the TimedLaunch name of each step form (conv_mfma_f32.hip's launch helpers); the sliced forms
# launch once per slice
LAUNCH_NAME = dict(stem='mfma_stem_f32', stem_conv1_pool='mfma_stem_conv1_pool_f32', conv3='mfma_conv3_f32',
                   conv3_conv1='mfma_conv3_conv1_f32', conv3_conv1_pool='mfma_conv3_conv1_pool_f32',
                   conv1='mfma_conv1_f32', atrous='mfma_atrous3_f32', deconv='mfma_deconv2_f32',
                   down='mfma_down2_f32', pool='mfma_pool_f32', add='mfma_add_f32', concat='mfma_concat_f32')


def build_driver(tmp_path, sanitize=False):
    """the driver's path, or None without a host compiler.  The header is built alone: of the project
    only fplhip.h, which it includes by its place in the tree, is in reach"""
    cxx = host_cxx()
    if not cxx:
        return None
    csrc, inc = tmp_path / 'flypylib_amd' / 'csrc', tmp_path / 'include'
    csrc.mkdir(parents=True)
    inc.mkdir()
    shutil.copy(os.path.join(ROOT, 'flypylib_amd', 'csrc', 'mfma_f32_plan.h'), str(csrc))
    shutil.copy(os.path.join(ROOT, 'include', 'fplhip.h'), str(inc))
    src = tmp_path / 'mfma_f32_plan_driver.cpp'
    src.write_text(DRIVER)
    exe = tmp_path / 'mfma_f32_plan_driver'
    flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g'] if sanitize else []
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror'] + flags + ['-I' + str(csrc), '-o', str(exe), str(src)],
                   check=True)
    return str(exe)


def program_text(ops, out_tensor, unfused=False):
    n_tensors = 1 + max(o['dst'] for o in ops)
    head = '%d %d %d %d' % (int(unfused), n_tensors, out_tensor, len(ops))
    body = ' '.join('%d %d %d %d %d %d %d %d %d %d %d %d %d %d' % ((o['kind'], o['src0'], o['src1'], o['dst'], o['k'],
                                                                    o['cin'], o['cout'], o['act']) + tuple(o['p']))
                    for o in ops)
    return head + ' ' + body + '\n'


def ask_plans(exe, programs):
    """programs: (ops, out_tensor, unfused) -> (list of plans, the header's constants)"""
    text = ''.join(program_text(*p) for p in programs)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, check=True, text=True).stdout
    lines = out.strip().split('\n')
    assert len(lines) == len(programs) + 1
    return [json.loads(ln) for ln in lines[1:]], json.loads(lines[0])


def plan_launches(plan):
    """{TimedLaunch name: launches} of a plan's steps"""
    n = {}
    for s in plan['steps']:
        name = LAUNCH_NAME[s['form']]
        n[name] = n.get(name, 0) + (len(s['slices']) if s['form'] in ('conv3', 'atrous') else 1)
    return n


# ---- the sweep --------------------------------------------------------------------------------
CHANNELS = (1, 5, 16, 17, 32, 48, 64, 65, 96, 128, 130, 192, 257)
COMMON = (16, 32, 48, 64)          # the widths drawn two times in three: most kernels exist for them
SWEEP_SEED, SWEEP_N = 20261, 2000


def _op(kind, src0, dst, cin, cout, src1=-1, k=0, act=0, p=(0,) * 6):
    return dict(kind=kind, src0=src0, src1=src1, dst=dst, k=k, cin=cin, cout=cout, act=act, p=tuple(p))


def random_program(rng):
    """(ops, out_tensor): 2 to 8 ops over all nine kinds, channel-consistent, operands among the
    earlier tensors (mostly the latest), the output the last op's.  Chains that the fused kernels
    take (3x3x3 -> 1x1x1 of the same width -> pool) are begun on purpose now and then."""
    n_ops = int(rng.integers(2, 9))
    ch = [1]                                   # channels per tensor
    ops, queue = [], []

    def pick():
        return len(ch) - 1 if rng.random() < 0.7 else int(rng.integers(0, len(ch)))

    def width():
        return int(rng.choice(COMMON if rng.random() < 0.67 else CHANNELS))

    while len(ops) < n_ops:
        dst = len(ch)
        if queue:
            kind, c = queue.pop(0)
            src = dst - 1
        else:
            kind = int(rng.choice([OP_CONV] * 6 + [OP_POOL, OP_UP, OP_CROP, OP_CONCAT, OP_CONCAT, OP_ADD, OP_ADD,
                                                   OP_DECONV, OP_DECONV, OP_DOWN, OP_DILATED]))
            src, c = pick(), width()
        cin = ch[src]
        act = int(rng.integers(0, 2))
        if kind == OP_CONV:
            k = 3 if rng.random() < 0.5 else 1
            if k == 3 and cin == 1 and rng.random() < 0.5:
                c = int(rng.choice((5, 16, 32, 32, 48, 48, 64, 65)))
            ops.append(_op(OP_CONV, src, dst, cin, c, k=k, act=act if rng.random() < 0.9 else 2))
            if k == 3 and not queue and rng.random() < 0.6:
                queue.append((-1, c if rng.random() < 0.8 else width()))        # a 1x1x1 conv behind it
                if rng.random() < 0.6:
                    queue.append((OP_POOL, 0))
        elif kind == -1:
            ops.append(_op(OP_CONV, src, dst, cin, c, k=1, act=act))
        elif kind in (OP_DECONV, OP_DOWN):
            ops.append(_op(kind, src, dst, cin, c, k=2, act=act, p=(2, 2, 2, 0, 0, 0)))
        elif kind == OP_DILATED:
            ops.append(_op(kind, src, dst, cin, c, k=3, act=act, p=(2, 2, 2, 0, 0, 0)))
        elif kind == OP_POOL:
            f = 2 if rng.random() < 0.85 else int(rng.choice((1, 3)))
            ops.append(_op(kind, src, dst, cin, cin, p=(f, f, f, 0, 0, 0)))
        elif kind == OP_UP:
            f = int(rng.choice((1, 2, 2, 2, 3)))
            ops.append(_op(kind, src, dst, cin, cin, p=(f, f, f, 0, 0, 0)))
        elif kind == OP_CROP:
            c0 = int(rng.integers(0, 3))
            p = (c0,) * 6 if rng.random() < 0.85 else (c0, c0 + 1, c0, c0, c0, c0)
            ops.append(_op(kind, src, dst, cin, cin, p=p))
        elif kind == OP_CONCAT:
            s1 = pick()
            ops.append(_op(kind, src, dst, cin, cin + ch[s1], src1=s1))
        else:
            same = [t for t in range(len(ch)) if ch[t] == cin and t != src] or [src]
            ops.append(_op(OP_ADD, src, dst, cin, cin, src1=int(rng.choice(same)), act=act))
        ch.append(ops[-1]['cout'])
    return ops, ops[-1]['dst']


def sweep():
    rng = np.random.default_rng(SWEEP_SEED)
    return [random_program(rng) for _ in range(SWEEP_N)]
