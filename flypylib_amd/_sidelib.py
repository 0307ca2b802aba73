"""What the ctypes bindings of the side libraries share (one _<key>capi.py per row of
csrc/build.py's SIDE_LIBRARIES): finding and loading the library, binding its SIGNATURES, the
ABI check, the cache, and turning an rc into the binding's error.

A binding module declares its constants, its error class and its SIGNATURES, makes one
SideLibrary of them and keeps `LIB_PATH`, `load_library` and `check` as names of its own.
"""
import ctypes as C
import importlib
import os

from .csrc import build


class SideLibrary:
    """`key`: of its row of build.SIDE_LIBRARIES, which holds the file under lib/ and the prefix
    of its exports; `error`: the RuntimeError subclass the binding raises;
    `hint`: what the not-found message says of the host path; `post_load(lib)`: a further
    check of a freshly bound library (it raises, or the library is kept)."""

    def __init__(self, key, error, signatures, abi_version, hint, post_load=None):
        _, _, self.prefix, _, self.name = next(r for r in build.SIDE_LIBRARIES if r[0] == key)
        self.error, self.signatures, self.abi_version = error, signatures, abi_version
        self.hint, self.post_load = hint, post_load
        self.path = os.path.join(build.LIB_DIR, self.name)
        self._lib = None

    def load(self, path=None):
        """dlopen the library and bind every declared symbol (no GPU needed)"""
        if self._lib is not None and path is None:
            return self._lib
        path = path or self.path
        if not os.path.exists(path):
            raise self.error('%s not found at %s - build it with `python -m flypylib_amd.csrc.build` '
                             '(%s)' % (self.name, path, self.hint))
        # one HIP runtime per process, shared with torch and libfplhip.so: the same preload
        # rule as _capi.load_library
        if not os.environ.get('FPL_NO_TORCH_PRELOAD'):
            try:
                import torch  # noqa: F401
            except Exception:       # noqa: BLE001
                pass
        lib = C.CDLL(path)
        for name, (res, args) in self.signatures.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        abi = getattr(lib, self.prefix + '_abi_version')()
        if abi != self.abi_version:
            raise self.error('%s ABI %d, binding expects %d' % (self.name, abi, self.abi_version))
        if self.post_load is not None:
            self.post_load(lib)
        self._lib = lib
        return lib

    def check(self, lib, rc):
        if rc != 0:
            last = getattr(lib, self.prefix + '_last_error')
            raise self.error((last() or b'').decode() or 'rc %d' % rc)


def bindings():
    """the binding modules of build.EAGER_BINDINGS"""
    return [importlib.import_module('%s._%scapi' % (__package__, key))
            for key in build.EAGER_BINDINGS]


def load_all():
    """every one of them loads and every declared symbol resolves (no GPU needed)"""
    for binding in bindings():
        binding.load_library()
