"""CPU: the slab and chunk planner of the fused vgg executors (csrc/vgg_plan.h), built alone
with the host C++ compiler and compared, case by case, with the arithmetic the four
executors carried as private copies before the header existed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from flypylib_amd import multi_gpu
from oracle import infer_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'flypylib_amd', 'csrc')

# One line in, one line out.  in: variant vox_bytes split_cap tile_z budget dz dy dx out_z zb ze
# n origins...; out: empty VZ VY VX fz_hi cz_lo cz_hi CY CX max_rows chunk size0 size1 size2
# c0:CZ ...  (sizes: P1, P2, 0 for vgg_like; H1, L3, Q for vgg_like2, as the executors
# allocate them; the split vgg_like executor adds x8::Tensor's read slack on top)
DRIVER = r'''
#include <cstdio>
#include <iostream>
#include "vgg_plan.h"
static void sizes(const VggPyramid &z, const VggPyramid &y, const VggPyramid &x, int64_t vox, int64_t b[3]) {
  b[0] = (int64_t)z.P1 * y.P1 * x.P1 * vox; b[1] = (int64_t)z.P2 * y.P2 * x.P2 * vox; b[2] = 0;
}
static void sizes(const Vgg2Pyramid &z, const Vgg2Pyramid &y, const Vgg2Pyramid &x, int64_t vox, int64_t b[3]) {
  b[0] = (int64_t)z.H * y.H * x.H * vox; b[1] = (int64_t)z.T3 * y.T3 * x.T3 * vox;
  b[2] = (int64_t)z.Q * y.Q * x.Q * vox;
}
int main() {
  long long variant, vox, cap, tz, budget, d[3], out_z, zb, ze, n;
  while (std::cin >> variant >> vox >> cap >> tz >> budget >> d[0] >> d[1] >> d[2] >> out_z >> zb >> ze >> n) {
    std::vector<int32_t> org(n);
    for (auto &o : org) std::cin >> o;
    const int64_t dims[3] = {d[0], d[1], d[2]};
    const VggSlab s = vgg_slab(dims, org, (int32_t)out_z, (int32_t)zb, (int32_t)ze, variant == 1 ? 7 : 10);
    if (s.empty) { printf("1\n"); continue; }
    printf("0 %lld %lld %lld %lld %lld %lld %d %d", (long long)s.VZ, (long long)s.VY, (long long)s.VX,
           (long long)s.fz_hi, (long long)s.cz_lo, (long long)s.cz_hi, s.CY, s.CX);
    int64_t max_rows = 0, chunk, b[3];
    if (variant == 1) {
      const VggPyramid y(s.CY), x(s.CX);
      if (cap) max_rows = vgg_split_max_p1_rows(y.P1, x.P1, (int)tz);
      chunk = vgg_chunk_rows(budget, (int64_t)y.P1 * x.P1 * vox, VggPyramid(0).P1, s.cz_hi - s.cz_lo,
                             cap ? vgg_split_chunk_cap(max_rows) : 0);
      sizes(VggPyramid(chunk), y, x, vox, b);
    } else {
      const Vgg2Pyramid y(s.CY), x(s.CX);
      chunk = vgg_chunk_rows(budget, ((int64_t)y.H * x.H + (int64_t)y.T3 * x.T3) * vox, Vgg2Pyramid(0).H,
                             s.cz_hi - s.cz_lo);
      sizes(Vgg2Pyramid(chunk), y, x, vox, b);
    }
    printf(" %lld %lld %lld %lld %lld", (long long)max_rows, (long long)chunk, (long long)b[0],
           (long long)b[1], (long long)b[2]);
    for (int64_t c0 = s.cz_lo; c0 < s.cz_hi; c0 += chunk)
      printf(" %lld:%lld", (long long)c0, (long long)std::min<int64_t>(chunk, s.cz_hi - c0));
    printf("\n");
  }
  return 0;
}
'''

GIB = 1 << 30
MIB = 1 << 20


def _cdiv(a, b):
    return -(-a // b)


def _parent_plan(variant, vox, split_cap, tile_z, budget, dims, org, out_z, zb, ze):
    """The executors' own arithmetic before vgg_plan.h, restated from their code: vgg_like
    (offset 7: P2 = C + 2, P1 = 2 P2 + 2, chunk by the P1 row, 6 fixed rows) and vgg_like2
    (offset 10: Q = C + 2, T3 = 2 Q + 2, H = T3 + 2, chunk by the H + T3 rows, 8 fixed rows);
    split vgg_like alone clips the chunk by the tile loader's 32-bit offsets."""
    off = 7 if variant == 1 else 10
    SZ, SY, SX = dims
    VZ, VY, VX = SZ - 2 * off, SY - 2 * off, SX - 2 * off
    if VZ <= 0 or VY <= 0 or VX <= 0 or zb >= ze:
        return None
    fz_lo = org[zb] - off
    fz_hi = min(org[ze - 1] - off + out_z, VZ)
    cz_lo, cz_hi = fz_lo // 4, _cdiv(fz_hi, 4)
    CY, CX = _cdiv(VY, 4), _cdiv(VX, 4)
    max_rows = 0
    if variant == 1:
        P2Y, P2X = CY + 2, CX + 2
        P1Y, P1X = 2 * P2Y + 2, 2 * P2X + 2
        p1_row = P1Y * P1X * vox
        chunk = max(4, (budget // p1_row - 6) // 2)
        chunk = min(chunk, cz_hi - cz_lo)
        chunk = (chunk + 3) // 4 * 4
        if split_cap:
            max_rows = (1 << 32) // 16 // (P1Y * P1X) - (tile_z + 2)
            chunk = min(chunk, max(4, ((max_rows - 6) // 2) // 4 * 4))
        sizes = [(2 * chunk + 6) * p1_row, (chunk + 2) * P2Y * P2X * vox, 0]
        planes = [p1_row, P2Y * P2X * vox, 0]

        def rows(cz):                                 # P1Z, P2Z of a chunk of cz coarse rows
            return [2 * (cz + 2) + 2, cz + 2, 0]
    else:
        QY, QX = CY + 2, CX + 2
        T3Y, T3X = 2 * QY + 2, 2 * QX + 2
        HY, HX = T3Y + 2, T3X + 2
        h_row, t_row = HY * HX * vox, T3Y * T3X * vox
        chunk = max(4, (budget // (h_row + t_row) - 8) // 2)
        chunk = min(chunk, cz_hi - cz_lo)
        chunk = (chunk + 3) // 4 * 4
        sizes = [(2 * chunk + 8) * h_row, (2 * chunk + 6) * t_row, (chunk + 2) * QY * QX * vox]
        planes = [h_row, t_row, QY * QX * vox]

        def rows(cz):                                 # HZ, T3Z, QZ
            return [2 * (cz + 2) + 2 + 2, 2 * (cz + 2) + 2, cz + 2]
    chunks = []
    c0 = cz_lo
    while c0 < cz_hi:
        chunks.append((c0, min(chunk, cz_hi - c0)))
        c0 += chunk
    return dict(fields=[VZ, VY, VX, fz_hi, cz_lo, cz_hi, CY, CX, max_rows, chunk], sizes=sizes,
                chunks=chunks, rows=rows, planes=planes,
                p1_plane_voxels=P1Y * P1X if variant == 1 else 0)


def _host_cxx():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def _scratch_defaults():
    """the two default budgets, read from common.h: (plain vgg_like, the other three)"""
    text = open(os.path.join(CSRC, 'common.h')).read()
    vals = []
    for name in ('FPL_VGG_SCRATCH_PLAIN_VGG', 'FPL_VGG_SCRATCH_DEFAULT'):
        m = re.search(r'constexpr int64_t %s = \(int64_t\)(\d+) << (\d+);' % name, text)
        assert m, name
        vals.append(int(m.group(1)) << int(m.group(2)))
    return tuple(vals)


def test_scratch_defaults_are_the_executors_own():
    assert _scratch_defaults() == (48 * GIB, 64 * GIB)


def test_planner_equals_the_executors_arithmetic(tmp_path):
    cxx = _host_cxx()
    if not cxx:
        pytest.skip('no host C++ compiler')
    src = tmp_path / 'plan_driver.cpp'
    src.write_text(DRIVER)
    exe = tmp_path / 'plan_driver'
    # vgg_plan.h alone, by the host compiler: no HIP, no other project header in reach
    inc = tmp_path / 'inc'
    inc.mkdir()
    shutil.copy(os.path.join(CSRC, 'vgg_plan.h'), str(inc))
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + str(inc), '-o', str(exe), str(src)],
                   check=True)
    m = re.search(r'constexpr int BZ = (\d+)', open(os.path.join(CSRC, 'vgg_split_lds.h')).read())
    assert m
    tile_z = int(m.group(1)) + 2                     # x8::TZ = BZ + 2
    plain_default, default = _scratch_defaults()

    extents = (46, 102, 103, 190, 270, 520, 1024)
    volumes = [(e,) * 3 for e in extents]
    volumes += [(150, 118, 134), (46, 1024, 103), (520, 270, 190), (1024, 46, 520), (103, 102, 1024),
                (14, 60, 60), (21, 30, 40), (20, 20, 20), (15, 15, 15),
                # planes large enough for the split path's 32-bit cap to cut the chunk
                (600, 2048, 2048), (1024, 3000, 2600)]
    # (variant, voxel bytes, split cap, tile edge, border): plain 16-bit operands carry 96 B per
    # voxel, split halves 192 B
    execs = [(1, 96, 0, 102, 7), (1, 192, 1, 102, 7), (2, 96, 0, 100, 10), (2, 192, 0, 100, 10)]
    cases = []
    for dims in volumes:
        for variant, vox, cap, tile, off in execs:
            if min(dims) > 2 * off:
                locs, _, _ = infer_oracle.tile_lattice(dims, (tile,) * 3, (off,) * 3)
                org = [int(v) for v in np.unique(locs[0])]
                assert len(org) == multi_gpu.n_tile_rows(dims[0], tile, off)
            else:
                org = [off]                           # never read: the slab is empty
            slabs = sorted({z for parts in (1, 2, 3, 5) for z in multi_gpu.slab_partition(len(org), parts)})
            dflt = plain_default if (variant, vox) == (1, 96) else default
            for zb, ze in slabs:
                for budget in (1 * MIB, 2 * MIB, 8 * MIB, dflt):
                    cases.append((variant, vox, cap, tile_z, budget, dims, org, tile - 2 * off, zb, ze))
    text = ''.join('%d %d %d %d %d %d %d %d %d %d %d %d %s\n'
                   % (c[0], c[1], c[2], c[3], c[4], c[5][0], c[5][1], c[5][2], c[7], c[8], c[9], len(c[6]),
                      ' '.join(map(str, c[6]))) for c in cases)
    out = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, check=True, text=True).stdout
    lines = out.strip().split('\n')
    assert len(lines) == len(cases)
    n_multi = n_capped = n_empty = 0
    for c, line in zip(cases, lines):
        want = _parent_plan(*c)
        tok = line.split()
        if want is None:
            assert tok == ['1'], (c, line)
            n_empty += 1
            continue
        assert tok[0] == '0', (c, line)
        assert [int(t) for t in tok[1:11]] == want['fields'], (c, line)
        assert [int(t) for t in tok[11:14]] == want['sizes'], (c, line)
        chunks = [tuple(int(v) for v in t.split(':')) for t in tok[14:]]
        assert chunks == want['chunks'], (c, line)
        # ... and what the formulas are for
        cz_lo, cz_hi, chunk = want['fields'][4], want['fields'][5], want['fields'][9]
        assert chunks and chunks[0][0] == cz_lo and chunks[-1][0] + chunks[-1][1] == cz_hi
        assert all(a[0] + a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        assert all(n > 0 and n % 4 == 0 for _, n in chunks[:-1]) and chunks[-1][1] > 0
        for _, n in chunks:
            assert n <= chunk
            assert all(r * p <= s for r, p, s in zip(want['rows'](n), want['planes'], want['sizes']))
        max_rows = want['fields'][8]
        if c[2] and max_rows >= 14:                   # below 14 the executor refuses the volume
            # A tile load addresses a pass's hi AND lo part plane (16 B per voxel each) from one
            # base in the hi plane: the lo plane's end plus the tile's reach of tile_z + 2 rows
            # must lie within 32 bits of it, i.e. one part plane plus that reach below 4 GiB
            for _, n in chunks:
                assert (want['rows'](n)[0] + tile_z + 2) * want['p1_plane_voxels'] * 16 <= 1 << 32, (c, line)
            uncapped = (min(max(4, (c[4] // want['planes'][0] - 6) // 2), cz_hi - cz_lo) + 3) // 4 * 4
            n_capped += chunk < uncapped
        n_multi += len(chunks) >= 3
    assert n_multi > 100 and n_capped > 0 and n_empty > 0     # the sweep reaches every branch
