"""Build libfplhip.so and the side libraries for gfx950 (MI355X) with hipcc, in-tree.

    python -m flypylib_amd.csrc.build [--force] [-j N]

Each .hip translation unit is compiled to build/<name>.o and linked into
flypylib_amd/lib/libfplhip.so.  An object is reused only when the SHA-256 of what it
was built from (its source, every header, the compiler flags) matches the stamp next
to it - modification times say nothing on a tree that ships objects, and the driver's
build check must compile what it ships.  hipcc cross-compiles without a GPU, so this
runs in the CPU-only build container.

Every row of SIDE_LIBRARIES is a library of its own: its sources live in a directory under
csrc/, are compiled with the same flags and stamps, and its version script exports its own
prefix only - libfplhip.so's export list stays the fpl_* names of include/fplhip.h.  The
side libraries share the headers of csrc/side/ (the C shell of side_abi.h, the device code of
side_device.h), which are part of their stamps and not of libfplhip.so's.

SIDE_LIBRARIES is the one table of them.  A row is a library's key (its binding is
flypylib_amd/_<key>capi.py, which reads the library's name and prefix from its row), its source
directory, its export prefix, its public header and its file under lib/.  build() and
build_side() walk the table.  Two facts are stated by key beside it:

SHARES_CSRC_HEADERS - libfplseg.so's source shares csrc/seg_box.h with libfplhip.so, so the
headers of csrc/ are part of its stamp and of no other row's.

EAGER_BINDINGS - the bindings _sidelib.bindings() / load_all() answer for, which the driver's
build check loads: the stages of the training round (batch, mine, labels).  Every other binding
loads lazily, when a call asks for its device path.
"""
import argparse
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OBJ_DIR = os.path.join(HERE, 'build')
LIB_DIR = os.path.join(os.path.dirname(HERE), 'lib')
LIB = os.path.join(LIB_DIR, 'libfplhip.so')
# key (its binding is flypylib_amd/_<key>capi.py), source directory under csrc/ (and the
# stem of its objects), export prefix, public header under include/, library under lib/
SIDE_LIBRARIES = (
    ('batch', 'batchgen', 'fplb', 'fplbatch.h', 'libfplbatch.so'),     # device batch generators
    ('mine', 'mine', 'fplm', 'fplmine.h', 'libfplmine.so'),            # hard-example mining
    ('labels', 'labels', 'fpll', 'fpllabels.h', 'libfpllabels.so'),    # write_labels_mask
    ('plan', 'plan', 'fplp', 'fplplan.h', 'libfplplan.so'),            # plan_bricks on the device
    ('match', 'match', 'fple', 'fplmatch.h', 'libfplmatch.so'),        # obj_pr's close pairs
    ('near', 'near', 'fpln', 'fplnear.h', 'libfplnear.so'),            # rm_tbar_multi_pred's close pairs
    ('assign', 'assign', 'fpla', 'fplassign.h', 'libfplassign.so'),    # obj_pr's matching, solved
    ('seg', 'seg', 'fpls', 'fplseg.h', 'libfplseg.so'),                # labels of a resident volume
    ('merge', 'merge', 'fplg', 'fplmerge.h', 'libfplmerge.so'),        # rm_tbar_multi_pred's merge loop
    ('valid', 'valid', 'fplv', 'fplval.h', 'libfplval.so'),            # held-out validation's sums
    ('clahe', 'clahe', 'fplc', 'fplclahe.h', 'libfplclahe.so'),        # fplutils.clahe
    ('roi', 'roi', 'fplr', 'fplroi.h', 'libfplroi.so'),                # BlockRoi, roi_to_substacks
)
# the rows whose sources include headers of csrc/ itself (seg_box.h), by key
SHARES_CSRC_HEADERS = ('seg',)
# the rows whose bindings _sidelib.load_all() loads, by key; the others load lazily
EAGER_BINDINGS = ('batch', 'mine', 'labels')
ARCH = 'gfx950'
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CXXFLAGS = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC',
            '-fvisibility=hidden', '-fvisibility-inlines-hidden',
            '-ffp-contract=on', '-Wall', '-Wno-unused-function',
            '-Wno-unused-but-set-variable', '-Wno-unused-variable',
            '-Wno-unused-value', '-Wno-unused-result']
# throw-away timing experiments only (e.g. FPL_EXTRA_CXXFLAGS=-DFPL_EXP_NOMATH=1)
CXXFLAGS += os.environ.get('FPL_EXTRA_CXXFLAGS', '').split()


# translation units built a second time with -DFPL_F16 (IEEE-half operands instead of
# bfloat16; mfma_util.h)
DUAL_PRECISION = ('vgg_fused.hip', 'conv_mfma.hip')
# ... and a third time on SPLIT IEEE-half operands (hi + lo per value; -DFPL_SPLIT):
# the U-Net executor (vgg_like's split kernels are a file of their own, vgg_split.hip)
SPLIT_BUILD = ('conv_mfma.hip',)


def _sources():
    """(source file, object stem, extra flags)"""
    out = []
    for f in sorted(os.listdir(HERE)):
        if f.endswith('.hip'):
            out.append((f, f[:-4], []))
            if f in DUAL_PRECISION:
                out.append((f, f[:-4] + '_f16', ['-DFPL_F16=1']))
            if f in SPLIT_BUILD:
                out.append((f, f[:-4] + '_f16s', ['-DFPL_F16=1', '-DFPL_SPLIT=1']))
    return out


def _digest(paths):
    """one digest over every header a translation unit may include"""
    h = hashlib.sha256()
    for p in paths:
        h.update(os.path.basename(p).encode() + b'\0')
        h.update(open(p, 'rb').read())
    return h.hexdigest()


def _local_headers(d):
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith('.h'))


def _compile(unit, force, hdr_digest, src_dir=HERE):
    src, stem, extra = unit
    obj = os.path.join(OBJ_DIR, stem + '.o')
    stamp = obj + '.sha256'
    sp = os.path.join(src_dir, src)
    h = hashlib.sha256()
    h.update(open(sp, 'rb').read())
    h.update(hdr_digest.encode())
    h.update(' '.join(CXXFLAGS + extra).encode())
    want = h.hexdigest()
    if (not force and os.path.exists(obj) and os.path.exists(stamp)
            and open(stamp).read().strip() == want):
        return obj, None
    cmd = [HIPCC] + CXXFLAGS + extra + ['-c', sp, '-o', obj]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    if r.returncode != 0:
        if os.path.exists(stamp):
            os.remove(stamp)
        raise RuntimeError('hipcc failed for %s:\n%s' % (stem, r.stdout))
    with open(stamp, 'w') as f:
        f.write(want + '\n')
    return obj, r.stdout


def _build_library(lib, exports, srcs, src_dir, hdr_digest, force, jobs, verbose):
    """compile `srcs` (stale objects only) and link them into `lib`, whose version script
    exports the `exports` pattern and nothing else"""
    os.makedirs(OBJ_DIR, exist_ok=True)
    os.makedirs(LIB_DIR, exist_ok=True)
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        results = list(ex.map(lambda s: _compile(s, force, hdr_digest, src_dir), srcs))
    objs = [o for o, _ in results]
    rebuilt = [u[1] for u, (_, out) in zip(srcs, results) if out is not None]
    for u, (_, out) in zip(srcs, results):
        if out and verbose and out.strip():
            print('[%s]\n%s' % (u[1], out.strip()))
    # the library carries the digest of the objects it was linked from
    lh = hashlib.sha256()
    for o in objs:
        lh.update(open(o + '.sha256').read().encode())
    lib_want = lh.hexdigest()
    lib_stamp = lib + '.sha256'
    if (rebuilt or not os.path.exists(lib) or not os.path.exists(lib_stamp)
            or open(lib_stamp).read().strip() != lib_want):
        # the export list = the C entry points the library's header declares, nothing else
        # (the C++ internals are hidden by -fvisibility=hidden, libstdc++'s template
        # instances - default visibility by their own headers - by this version script)
        vs = os.path.join(OBJ_DIR, os.path.basename(lib) + '.map')
        with open(vs, 'w') as f:
            f.write('{ global: %s; local: *; };\n' % exports)
        cmd = [HIPCC, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-Wl,--version-script=' + vs,
               '-o', lib] + objs
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True)
        if r.returncode != 0:
            raise RuntimeError('link failed:\n%s' % r.stdout)
        with open(lib_stamp, 'w') as f:
            f.write(lib_want + '\n')
        if verbose:
            print('linked %s (%d objects, rebuilt: %s)' % (
                os.path.relpath(lib, ROOT), len(objs), ', '.join(rebuilt) or '-'))
    elif verbose:
        print('%s is up to date' % os.path.relpath(lib, ROOT))
    return lib


def build(force=False, jobs=4, verbose=True):
    inc = os.path.join(ROOT, 'include')
    _build_library(LIB, 'fpl_*', _sources(), HERE,
                   _digest(_local_headers(HERE) + [os.path.join(inc, 'fplhip.h')]),
                   force, jobs, verbose)
    for row in SIDE_LIBRARIES:
        build_side(row[0], force, jobs, verbose)
    return LIB


def build_side(key, force=False, jobs=4, verbose=True):
    """one row of SIDE_LIBRARIES: same flags, same SHA-stamped rebuild, a version script that
    exports the row's prefix only"""
    _, sub, prefix, header, lib = next(r for r in SIDE_LIBRARIES if r[0] == key)
    src_dir, inc = os.path.join(HERE, sub), os.path.join(ROOT, 'include')
    srcs = [(f, '%s_%s' % (sub, f[:-4]), ['-I' + inc])
            for f in sorted(os.listdir(src_dir)) if f.endswith('.hip')]
    return _build_library(os.path.join(LIB_DIR, lib), prefix + '_*', srcs, src_dir,
                          _digest(_local_headers(src_dir)
                                  + _local_headers(os.path.join(HERE, 'side'))
                                  + (_local_headers(HERE) if key in SHARES_CSRC_HEADERS else [])
                                  + [os.path.join(inc, header)]),
                          force, jobs, verbose)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--force', action='store_true')
    ap.add_argument('-j', type=int, default=4)
    a = ap.parse_args()
    try:
        build(a.force, a.j)
    except RuntimeError as e:
        print(e, file=sys.stderr)
        sys.exit(1)
