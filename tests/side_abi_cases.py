"""The C ABI checks every side library gets (test_side_libraries.py): the export list is what
the public header declares, and every entry point is a guarded function-try-block."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'flypylib_amd', 'csrc')


def declared(header, prefix):
    """the names `include/<header>` declares, e.g. prefix 'fplm'"""
    hdr = open(os.path.join(ROOT, 'include', header)).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    return set(re.findall(r'\b(%s_[a-z0-9_]+)\s*\(' % prefix, hdr))


def check_exports(binding, header, prefix, n_exports):
    """header, binding and the library's dynamic symbol table name the same `n_exports`"""
    names = declared(header, prefix)
    assert names == set(binding.SIGNATURES) and len(names) == n_exports
    if shutil.which('nm') is None:
        pytest.skip('nm is not installed')
    out = subprocess.run(['nm', '-D', '--defined-only', binding.LIB_PATH],
                         stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    assert exported == names, exported ^ names
    return names


def closing(s, i, open_, close):
    assert s[i] == open_
    depth = 0
    while True:
        depth += {open_: 1, close: -1}.get(s[i], 0)
        if depth == 0:
            return i
        i += 1


def check_guarded(subdir, header, prefix, n_exports):
    """every entry point of csrc/<subdir> is a function-try-block; the int ones end in
    <PREFIX>_CATCH, which turns the exception into an rc; no threads"""
    d = os.path.join(CSRC, subdir)
    srcs = {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))
            if f.endswith(('.hip', '.h'))}
    upper = prefix.upper()
    # the library's own spelling is the shared shell's
    assert sum('#define %s_CATCH() SIDE_CATCH()\n' % upper in s for s in srcs.values()) == 1
    assert sum('#define %s_EXPORT SIDE_EXPORT\n' % upper in s for s in srcs.values()) == 1
    guarded = 0
    for name in sorted(declared(header, prefix)):
        defs = [(f, m) for f, s in srcs.items() if f.endswith('.hip')
                for m in re.finditer(r'^%s_EXPORT (?:int|const char \*)\s*%s\(' % (upper, name), s, re.M)]
        assert len(defs) == 1, (name, [f for f, _ in defs])
        f, m = defs[0]
        s = srcs[f]
        i = closing(s, m.end() - 1, '(', ')')
        assert s.startswith(') try {', i), '%s is not a function-try-block' % name
        end = closing(s, i + len(') try '), '{', '}')
        handler = ' catch (...) {' if name == prefix + '_last_error' else ' %s_CATCH()' % upper
        assert s.startswith(handler, end + 1), '%s: no handler after its body' % name
        guarded += 1
    assert guarded == n_exports
    srcs['side_abi.h'] = open(os.path.join(CSRC, 'side', 'side_abi.h')).read()
    # the shared shell belongs to no library: it spells no library's prefix
    assert not re.search(r'\bfpl[a-z]?_', srcs['side_abi.h'], re.I)
    assert not any('std::thread' in s for s in srcs.values())
