"""CPU: Conv3DTranspose on the graph executor - the compiler's resource report of every
FPLK(deconv2) instance in the three operand builds, and the host-side weight transposition
(csrc/deconv_pack.h) built alone with the host C++ compiler against numpy."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import deconv_gx_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'flypylib_amd', 'csrc')

BUILDS = {'bf16': (), 'f16': ('-DFPL_F16=1',), 'f16s': ('-DFPL_F16=1', '-DFPL_SPLIT=1')}
# DESIGN.md section 19, "The 16-bit and split-half kernel": KiB of LDS per instance (CIN, MB) = the
# TPB taps a workgroup holds times the KiB of one tap's fragments, (CIN / 32) * MB in the 16-bit
# builds and (CIN / 16) * 2 MB on split halves, TPB = the most taps (8, 4, 2, 1) within 64 KiB
LDS_KIB = {
    'bf16': {(32, 2): 16, (32, 4): 32, (64, 2): 32, (64, 4): 64, (96, 2): 48, (96, 4): 48, (128, 2): 64, (128, 4): 64},
    'f16': {(32, 2): 16, (32, 4): 32, (64, 2): 32, (64, 4): 64, (96, 2): 48, (96, 4): 48, (128, 2): 64, (128, 4): 64},
    'f16s': {(32, 2): 64, (32, 4): 64, (64, 2): 64, (64, 4): 64, (96, 2): 48, (96, 4): 48, (128, 2): 64, (128, 4): 64},
}


@pytest.mark.parametrize('build', sorted(BUILDS))
def test_no_deconv2_instance_spills_and_lds_is_as_designed(build):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from flypylib_amd.csrc import build as b
    if not shutil.which(b.HIPCC) and not os.path.exists(b.HIPCC):
        pytest.skip('hipcc not available')
    import kernel_resources
    res = {}
    for name, v in kernel_resources.kernel_resources('conv_mfma.hip', BUILDS[build]).items():
        m = re.search(r'deconv2_%sILi(\d+)ELi(\d+)EE' % build, name)
        if m:
            res[(int(m.group(1)), int(m.group(2)))] = v
    assert sorted(res) == sorted(LDS_KIB[build]), sorted(res)
    for key, v in sorted(res.items()):
        print(build, key, v)
        assert v['vgpr_spill_count'] == 0 and v['sgpr_spill_count'] == 0, (key, v)
        assert v['private_segment_fixed_size'] == 0, (key, v)
        assert v['group_segment_fixed_size'] == LDS_KIB[build][key] * 1024, (key, v)
        # two workgroups of four waves per CU: two waves per SIMD, 256 registers each
        assert v['vgpr_count'] + v['agpr_count'] <= 256, (key, v)


DRIVER = r'''
#include <cstdio>
#include <vector>
#include "deconv_pack.h"
// in (stdin, binary): int32 cin, cout, cin_p, cout_p; float K[8 * cout * cin], scale[cout], shift[cout]
// out (stdout, binary): per tap the arena of fpl_deconv_tap_arena
int main() {
  int h[4];
  if (fread(h, sizeof(int), 4, stdin) != 4) return 2;
  const int cin = h[0], cout = h[1], cin_p = h[2], cout_p = h[3];
  std::vector<float> K((size_t)8 * cout * cin), sc(cout), sh(cout);
  if (fread(K.data(), sizeof(float), K.size(), stdin) != K.size()) return 3;
  if (fread(sc.data(), sizeof(float), cout, stdin) != (size_t)cout) return 4;
  if (fread(sh.data(), sizeof(float), cout, stdin) != (size_t)cout) return 5;
  std::vector<float> ap((size_t)cin_p * cout_p + 2 * (size_t)cout_p, -7.f);
  for (int tap = 0; tap < 8; ++tap) {
    fpl_deconv_tap_arena(K.data(), sc.data(), sh.data(), cin, cout, tap, cin_p, cout_p, ap.data());
    fwrite(ap.data(), sizeof(float), ap.size(), stdout);
  }
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
    d = tmp_path_factory.mktemp('deconv_pack')
    (d / 'driver.cpp').write_text(DRIVER)
    inc = d / 'inc'
    inc.mkdir()
    shutil.copy(os.path.join(CSRC, 'deconv_pack.h'), str(inc))      # alone: no HIP, no other project header
    exe = d / 'driver'
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I' + str(inc), '-o', str(exe),
                    str(d / 'driver.cpp')], check=True)
    return str(exe)


@pytest.mark.parametrize('cin,cout', [(24, 8), (96, 48)])
def test_tap_matrices_are_the_numpy_transposition(driver, cin, cout):
    rng = np.random.default_rng(cin)
    cin_p, cout_p = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
    K = rng.standard_normal((2, 2, 2, cout, cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.standard_normal(cout).astype(np.float32)
    blob = np.array([cin, cout, cin_p, cout_p], np.int32).tobytes() + K.tobytes() + scale.tobytes() + shift.tobytes()
    r = subprocess.run([driver], input=blob, stdout=subprocess.PIPE, check=True)
    got = np.frombuffer(r.stdout, np.float32).reshape(8, cin_p * cout_p + 2 * cout_p)
    for a in range(2):
        for b in range(2):
            for c in range(2):
                want = np.zeros((cin_p, cout_p), np.float32)
                want[:cin, :cout] = K[a, b, c].T                   # [cout][cin] -> [cin][cout]
                tap = got[4 * a + 2 * b + c]
                assert np.array_equal(tap[:cin_p * cout_p].reshape(cin_p, cout_p), want)
                assert cout_p > cout and not tap[:cin_p * cout_p].reshape(cin_p, cout_p)[:, cout:].any()
                s, h = tap[cin_p * cout_p:cin_p * cout_p + cout_p], tap[cin_p * cout_p + cout_p:]
                assert np.array_equal(s[:cout], scale) and np.all(s[cout:] == 1.0)
                assert np.array_equal(h[:cout], shift) and not h[cout:].any()


def test_unet_t3_shapes_and_the_lowered_program():
    """the helper network: sizes as stated, rf_offset 4, and the lowered program holds the layer
    between the pooled convolution and the concatenation"""
    from flypylib_amd.program import OP_CONV, OP_DECONV
    g, rf, sz, _ = gc.unet_t3()
    assert rf == (9, 4, 1) and sz == (24, 24, 24) and g.output.size == (16, 16, 16)
    ops = g.lower_inference()[0]
    d = [o for o in ops if o['kind'] == OP_DECONV]
    assert len(d) == 1 and (d[0]['cin'], d[0]['cout'], d[0]['k']) == (32, 16, 2)
    assert sum(o['kind'] == OP_CONV for o in ops) == 4
    for cin, cout in ((16, 8), (128, 64)):
        for ep in gc.EPILOGUES:
            lg, off = gc.layer_alone(cin, cout, 1, ep)
            assert lg.output.size == (gc.tile_of(cin) - 2 * off,) * 3
