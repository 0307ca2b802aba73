"""The scaffold the side libraries share (no GPU): the loader of flypylib_amd/_sidelib.py as
each binding uses it, and csrc/side/side_abi.h driven by a host program of its own."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__
from flypylib_amd import _batchcapi, _labelscapi, _minecapi, _sidelib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# binding, its error class, the library, a refused raw call and the message it leaves
BINDINGS = {
    'batch': (_batchcapi, _batchcapi.FplBatchError, 'libfplbatch.so',
              lambda lib: lib.fplb_struct_sizes(None, None), 'fplb_struct_sizes: null argument'),
    'mine': (_minecapi, _minecapi.FplMineError, 'libfplmine.so',
             lambda lib: lib.fplm_voxel_loss(None, None, None, None, None, 0, 0.0, 0.0, 0, 0.0, 0.0,
                                             None, None),
             'fplm_voxel_loss: null pointer argument'),
    'labels': (_labelscapi, _labelscapi.FplLabelsError, 'libfpllabels.so',
               lambda lib: lib.fpll_labels_mask(None, None, 0, None, None, 0, None, 0, 0, 0, None,
                                                None, None),
               'fpll_labels_mask: null pointer argument'),
}


@pytest.fixture(params=sorted(BINDINGS))
def binding(request):
    return BINDINGS[request.param]


def test_a_missing_library_is_the_bindings_own_error(binding):
    mod, error, libname, _, _ = binding
    assert issubclass(error, RuntimeError) and error.__bases__ == (RuntimeError,)
    with pytest.raises(error) as e:
        mod.load_library('/nonexistent/x.so')
    text = str(e.value)
    assert text.startswith('%s not found at /nonexistent/x.so' % libname)
    assert 'python -m flypylib_amd.csrc.build' in text and 'no host fallback' in text
    assert os.path.basename(mod.LIB_PATH) == libname


def test_the_library_is_loaded_once(binding):
    mod = binding[0]
    assert mod.load_library() is mod.load_library()


def test_every_declared_symbol_is_bound(binding):
    mod = binding[0]
    lib = mod.load_library()
    assert len(mod.SIGNATURES) >= 3
    for name, (res, args) in mod.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_check_raises_the_librarys_message(binding):
    mod, error, _, refused, message = binding
    lib = mod.load_library()
    mod.check(lib, 0)
    assert refused(lib) == 1
    with pytest.raises(error) as e:
        mod.check(lib, 1)
    assert str(e.value) == message


def test_build_loads_every_binding():
    """__graft_entry__.build goes through _sidelib.load_all, which covers the build's table"""
    assert '_sidelib.load_all()' in inspect.getsource(__graft_entry__.build)
    assert {m.__name__ for m in _sidelib.bindings()} == {b[0].__name__ for b in BINDINGS.values()}


DRIVER = r'''
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>

#include "side_abi.h"

#define EXPECT(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int throws_runtime_error() try {
  throw std::runtime_error("x");
} SIDE_CATCH()

static int throws_int() try {
  throw 7;
} SIDE_CATCH()

int main() {
  EXPECT(side_err[0] == 0);
  EXPECT(side_fail("%s: %d of %lld", "fn", 3, 1ll << 40) == 1);
  EXPECT(!strcmp(side_err, "fn: 3 of 1099511627776"));

  const std::string big(2000, 'a');
  EXPECT(side_fail("%s", big.c_str()) == 1);
  EXPECT(sizeof(side_err) == 512 && strlen(side_err) == 511);
  EXPECT(std::string(side_err) == std::string(511, 'a'));

  EXPECT(throws_runtime_error() == 1);
  EXPECT(!strcmp(side_err, "throws_runtime_error: C++ exception: x"));
  EXPECT(throws_int() == 1);
  EXPECT(!strcmp(side_err, "throws_int: unknown C++ exception"));

  bool other_empty = false;
  std::thread([&] { other_empty = side_err[0] == 0; side_fail("other"); }).join();
  EXPECT(other_empty);
  EXPECT(!strcmp(side_err, "throws_int: unknown C++ exception"));

  EXPECT(aligned((const void *)0, 16) && aligned((const void *)256, 16));
  EXPECT(aligned((const void *)260, 4) && !aligned((const void *)260, 8));
  EXPECT(!aligned((const void *)257, 2) && aligned((const void *)257, 1));

  int64_t n = -1;
  const int64_t under[3] = {1290, 1290, 1290};
  EXPECT(volume_voxels("fn", under, "the brick tables", "render it in parts", &n) == 0);
  EXPECT(n == 2146689000ll);
  const int64_t top[3] = {2147483647, 1, 1};
  EXPECT(volume_voxels("fn", top, "the brick tables", "render it in parts", &n) == 0);
  EXPECT(n == 2147483647ll);
  n = -1;
  const int64_t over[3] = {2048, 1024, 1024};
  EXPECT(volume_voxels("fn", over, "int32 rows and counts", "mine it in parts", &n) == 1);
  EXPECT(n == -1);
  EXPECT(!strcmp(side_err, "fn: a volume of (2048,1024,1024) voxels exceeds the 2^31 - 1 voxels "
                           "int32 rows and counts can index; mine it in parts"));
  const int64_t axis[3] = {1, 1ll << 31, 1};
  EXPECT(volume_voxels("fn", axis, "the brick tables", "render it in parts", &n) == 1);
  EXPECT(n == -1);
  EXPECT(!strcmp(side_err, "fn: a volume of (1,2147483648,1) voxels exceeds the 2^31 - 1 voxels "
                           "the brick tables can index; render it in parts"));

  EXPECT(SIDE_INT32_MAX == 2147483647ll);
  side_fail("untouched");
  EXPECT(in_int32_range("fn", "n_gt", 1, 1) == 0);
  EXPECT(in_int32_range("fn", "n_gt", 2147483647ll, 1) == 0);
  EXPECT(in_int32_range("fn", "capacity", 0, 0) == 0);
  EXPECT(in_int32_range("fn", "capacity", 2147483647ll, 0) == 0);
  EXPECT(!strcmp(side_err, "untouched"));
  EXPECT(in_int32_range("fn", "n_gt", 1ll << 31, 1) == 1);
  EXPECT(!strcmp(side_err, "fn: n_gt 2147483648 must lie in [1, 2^31 - 1]"));
  EXPECT(in_int32_range("fn", "n_gt", 0, 1) == 1);
  EXPECT(!strcmp(side_err, "fn: n_gt 0 must lie in [1, 2^31 - 1]"));
  EXPECT(in_int32_range("fn", "capacity", -1, 0) == 1);
  EXPECT(!strcmp(side_err, "fn: capacity -1 must lie in [0, 2^31 - 1]"));
  EXPECT(in_int32_range("fn", "capacity", 1ll << 31, 0) == 1);
  EXPECT(!strcmp(side_err, "fn: capacity 2147483648 must lie in [0, 2^31 - 1]"));
  puts("side_abi ok");
  return 0;
}
'''


def _host_cxx():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_side_abi_header_by_a_host_driver(tmp_path):
    """side_abi.h alone, by the host compiler under ASan and UBSan: no HIP header in reach"""
    cxx = _host_cxx()
    if not cxx:
        pytest.skip('no host C++ compiler')
    src = tmp_path / 'side_driver.cpp'
    src.write_text(DRIVER)
    exe = tmp_path / 'side_driver'
    inc = tmp_path / 'inc'
    inc.mkdir()
    shutil.copy(os.path.join(ROOT, 'flypylib_amd', 'csrc', 'side', 'side_abi.h'), str(inc))
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-pthread',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I' + str(inc),
                    '-o', str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'side_abi ok', r.stdout
    # the two messages the libraries pass are the ones their sources spell
    for sub, what, advice in (('mine', 'int32 rows and counts', 'mine it in parts'),
                              ('labels', 'the brick tables', 'render it in parts')):
        text = open(os.path.join(ROOT, 'flypylib_amd', 'csrc', sub, sub + '.hip')).read()
        assert 'volume_voxels(fn, dims, "%s", "%s", &' % (what, advice) in text
    # the one block scan is csrc/side/side_device.h's, which belongs to no library either
    for sub in ('mine', 'match', 'near', 'assign'):
        text = open(os.path.join(ROOT, 'flypylib_amd', 'csrc', sub, sub + '.hip')).read()
        assert 'side_scan_kernel' in text and 'void scan_kernel(' not in text, sub
    device = open(os.path.join(ROOT, 'flypylib_amd', 'csrc', 'side', 'side_device.h')).read()
    assert not re.search(r'\bfpl[a-z]?_', device, re.I)
