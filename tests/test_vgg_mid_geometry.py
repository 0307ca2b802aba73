"""CPU: the block orientations of the split vgg_like mid kernel (csrc/vgg_plan.h: MidGeo, mid_voxel,
mid_slot_voxel, mid_tap_slot, vgg_mid_plan), built alone with the host C++ compiler.  The kernels
(csrc/vgg_split.hip: vggs_mid_pool_edge; csrc/vgg_split_lds.h: tile_dma_init_oriented,
ktab_init_oriented) take every address from these functions:

    tile gather   LDS slot s of a part plane  <-  P1 voxel  origin + mid_slot_voxel(s)
    B operand     slot(mid_voxel(wave, 0, c)) + slot(mid_voxel(0, sub, 0)) + mid_tap_slot(tap)
    store         pooled voxel  (origin + mid_voxel(wave, 0, c)) / 2  by the even lane of a pair

so a block enumerated here is the block the GPU runs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'flypylib_amd', 'csrc')
INTERIOR, XCOL, ZLAYER = 0, 1, 2

# "geo": per orientation one line  o BZ BY BX ZS slots, then per (wave, sub, c) one line
#   o wave sub c  z y x  lds_slot_of_tap_0..26 ; then per LDS slot  "s" o slot z y x
# "plan Z Y X reorient": per orientation  nbx nby nbz z0 x0
DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "vgg_plan.h"
int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "geo")) {
    for (int o = 0; o < 3; ++o) {
      const MidGeo G = mid_geo(o);
      printf("g %d %d %d %d %d %d\n", o, G.BZ, G.BY, G.BX, G.ZS, G.slots());
      for (int wave = 0; wave < 8; ++wave)
        for (int sub = 0; sub < 4; ++sub)
          for (int c = 0; c < 16; ++c) {
            const MidVox v = mid_voxel(o, wave, sub, c), v0 = mid_voxel(o, wave, 0, c), d = mid_voxel(o, 0, sub, 0);
            printf("v %d %d %d %d %d %d %d", o, wave, sub, c, v.z, v.y, v.x);
            for (int tap = 0; tap < 27; ++tap)
              printf(" %d", G.slot(v0.z, v0.y, v0.x) + G.slot(d.z, d.y, d.x) + mid_tap_slot(G, tap));
            printf("\n");
          }
      for (int s = 0; s < atoi(argv[2]); ++s) {
        const MidVox v = mid_slot_voxel(G, s);
        printf("s %d %d %d %d %d\n", o, s, v.z, v.y, v.x);
      }
    }
    return 0;
  }
  const MidPlan p = vgg_mid_plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]) != 0);
  for (int o = 0; o < 3; ++o)
    printf("%d %d %d %d %d\n", p.w[o].nbx, p.w[o].nby, p.w[o].nbz, p.w[o].z0, p.w[o].x0);
  return 0;
}
'''


def _host_cxx():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    cxx = _host_cxx()
    if not cxx:
        pytest.skip('no host C++ compiler')
    tmp = tmp_path_factory.mktemp('midgeo')
    src = tmp / 'geo_driver.cpp'
    src.write_text(DRIVER)
    inc = tmp / 'inc'
    inc.mkdir()
    shutil.copy(os.path.join(CSRC, 'vgg_plan.h'), str(inc))
    exe = tmp / 'geo_driver'
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + str(inc), '-o', str(exe), str(src)],
                   check=True)

    def run(*args):
        return subprocess.run([str(exe)] + [str(a) for a in args], stdout=subprocess.PIPE, check=True,
                              text=True).stdout.strip().split('\n')
    return run


def _plane_slots():
    """x8::PLANE: slots of one part plane of the LDS tile (vgg_split_lds.h)"""
    text = open(os.path.join(CSRC, 'vgg_split_lds.h')).read()
    assert 'constexpr int BZ = 8, BY = 4, BX = 16;' in text and 'constexpr int ZS = 118;' in text
    assert 'constexpr int PLANE = (TZ - 1) * ZS + TY * TX;' in text
    return 9 * 118 + 6 * 18


@pytest.fixture(scope='module')
def geo(driver):
    plane = _plane_slots()
    G, vox, slots = {}, {}, {}
    for line in driver('geo', plane):
        t = line.split()
        n = [int(v) for v in t[1:]]
        if t[0] == 'g':
            G[n[0]] = dict(B=tuple(n[1:4]), ZS=n[4], slots=n[5])
        elif t[0] == 'v':
            vox[tuple(n[:4])] = (tuple(n[4:7]), n[7:])
        else:
            slots[(n[0], n[1])] = tuple(n[2:5])
    return G, vox, slots, plane


def test_block_extents_and_tiles_fit_the_lds_plane(geo):
    G, _, _, plane = geo
    assert G[INTERIOR] == dict(B=(8, 4, 16), ZS=118, slots=plane)
    assert G[XCOL] == dict(B=(8, 16, 4), ZS=108, slots=1080)
    assert G[ZLAYER] == dict(B=(4, 8, 16), ZS=182, slots=1090)
    for o in G:
        assert G[o]['slots'] <= plane and np.prod(G[o]['B']) == 512


@pytest.mark.parametrize('o', [INTERIOR, XCOL, ZLAYER])
def test_every_output_voxel_once_and_every_tap_on_its_source(geo, o):
    G, vox, slots, plane = geo
    B = G[o]['B']
    # the gather: every voxel of the (B + 2)^3 tile has exactly one slot among the tile's slots,
    # and every slot of the plane (padding, slots behind the tile) loads a voxel of the tile
    src = {s: slots[(o, s)] for s in range(plane)}
    assert all(0 <= v[a] < B[a] + 2 for v in src.values() for a in range(3))
    tile = {}
    for s in range(G[o]['slots']):
        tile.setdefault(src[s], []).append(s)
    assert len(tile) == (B[0] + 2) * (B[1] + 2) * (B[2] + 2)
    seen = {}
    for wave in range(8):
        for sub in range(4):
            for c in range(16):
                v, taps = vox[(o, wave, sub, c)]
                assert all(0 <= v[a] < B[a] for a in range(3))
                assert v not in seen, (v, seen.get(v), (wave, sub, c))
                seen[v] = (wave, sub, c)
                # canonical tap order (dz, dy, dx): tap t reads the input voxel v + (dz, dy, dx)
                for t, s in enumerate(taps):
                    assert 0 <= s < G[o]['slots'], (wave, sub, c, t, s)
                    want = (v[0] + t // 9, v[1] + (t // 3) % 3, v[2] + t % 3)
                    assert src[s] == want and tile[want][0] == s, (wave, sub, c, t, s, src[s], want)
    assert len(seen) == 512
    # pooling: the four sub-steps of the lane pair (c, c + 1), c even, are one 2 x 2 x 2 window whose
    # even corner is sub-step 0 of lane c; the block's 64 pooled voxels come out once each
    pooled = set()
    for wave in range(8):
        for c in range(0, 16, 2):
            v0 = vox[(o, wave, 0, c)][0]
            assert all(x % 2 == 0 for x in v0)
            win = {vox[(o, wave, sub, cc)][0] for sub in range(4) for cc in (c, c + 1)}
            assert win == {(v0[0] + dz, v0[1] + dy, v0[2] + dx) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
            pooled.add(tuple(x // 2 for x in v0))
    assert len(pooled) == 64


def _plan(driver, Z, Y, X, reorient=1):
    return [tuple(int(v) for v in l.split()) for l in driver('plan', Z, Y, X, reorient)]


def _cdiv(a, b):
    return -(-a // b)


def test_plan_at_the_benchmark_volume(driver):
    """520^3: P2 = 129^3, 17 x 65 x 33 interior blocks of which the last column holds 1 of 8 pooled x
    and the last layer 1 of 4 pooled z"""
    assert _plan(driver, 129, 129, 129, 0) == [(17, 65, 33, 0, 0), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0)]
    assert _plan(driver, 129, 129, 129) == [(16, 65, 32, 0, 0), (1, 17, 33, 0, 256), (16, 33, 1, 256, 0)]
    # 1024^3: P2 = 255^3, 7 of 8 pooled x and 3 of 4 pooled z are live: no orientation has fewer blocks
    assert _plan(driver, 255, 255, 255) == [(32, 128, 64, 0, 0), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0)]


def test_plan_covers_p2_once_and_reorients_only_for_fewer_blocks(driver, geo):
    G = geo[0]
    n_x = n_z = n_both = n_keep = 0
    for Z in (3, 4, 5, 6, 7, 8, 13, 33):
        for Y in (3, 4, 9, 17, 40):
            for X in list(range(3, 20)) + [40, 41, 47]:
                plain = _plan(driver, Z, Y, X, 0)
                assert plain == [(_cdiv(X, 8), _cdiv(Y, 2), _cdiv(Z, 4), 0, 0)] + [(0,) * 5] * 2
                plan = _plan(driver, Z, Y, X)
                cover = np.zeros((Z, Y, X), np.int32)
                for o, (nbx, nby, nbz, z0, x0) in enumerate(plan):
                    bz, by, bx = (b // 2 for b in G[o]['B'])            # pooled extent of a block
                    assert z0 % 2 == 0 and x0 % 2 == 0
                    for k in range(nbz):
                        for j in range(nby):
                            for i in range(nbx):
                                cover[z0 // 2 + k * bz: z0 // 2 + (k + 1) * bz, j * by: (j + 1) * by,
                                      x0 // 2 + i * bx: x0 // 2 + (i + 1) * bx] += 1
                assert (cover == 1).all(), (Z, Y, X, plan)
                blocks = [w[0] * w[1] * w[2] for w in plan]
                total_plain = plain[0][0] * plain[0][1] * plain[0][2]
                assert sum(blocks) <= total_plain
                # an orientation is used only where it replaces MORE interior blocks than it issues
                nbx_p, nby_p, nbz_p = plain[0][:3]
                if blocks[XCOL]:
                    assert X % 8 and blocks[XCOL] < nby_p * nbz_p
                elif X % 8:
                    assert _cdiv(X % 8, 2) * _cdiv(Y, 8) * nbz_p >= nby_p * nbz_p
                nbx_m = plan[INTERIOR][0]
                if blocks[ZLAYER]:
                    assert Z % 4 and blocks[ZLAYER] < nbx_m * nby_p
                elif Z % 4 and nbx_m:
                    assert _cdiv(Z % 4, 2) * _cdiv(Y, 4) * nbx_m >= nbx_m * nby_p
                n_x += bool(blocks[XCOL]); n_z += bool(blocks[ZLAYER])
                n_both += bool(blocks[XCOL] and blocks[ZLAYER])
                n_keep += bool((X % 8 and not blocks[XCOL]) or (Z % 4 and not blocks[ZLAYER]))
                # the reads stay inside the tensor and x8::Tensor's slack behind it ((TZ + 1) planes
                # + 64 voxels, TZ = 10): P1 = 2 P2 + 2 per axis
                P1 = (2 * Z + 2, 2 * Y + 2, 2 * X + 2)
                for o, (nbx, nby, nbz, z0, x0) in enumerate(plan):
                    if nbx * nby * nbz:
                        B = G[o]['B']
                        last = (z0 + (nbz - 1) * B[0] + B[0] + 1, (nby - 1) * B[1] + B[1] + 1,
                                x0 + (nbx - 1) * B[2] + B[2] + 1)
                        idx = (last[0] * P1[1] + last[1]) * P1[2] + last[2]
                        assert idx < P1[0] * P1[1] * P1[2] + 11 * P1[1] * P1[2] + 64, (Z, Y, X, o)
    assert n_x > 50 and n_z > 50 and n_both > 20 and n_keep > 50          # the rule goes both ways
    # the rule by residue, on an extent large enough for the rounding not to matter
    for r in range(8):
        assert bool(_plan(driver, 40, 40, 40 + r)[XCOL][0]) == (1 <= r <= 6), r
    for r in range(4):
        assert bool(_plan(driver, 40 + r, 40, 40)[ZLAYER][0]) == (1 <= r <= 2), r
