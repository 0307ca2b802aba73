"""The one table of the side libraries (csrc/build.py's SIDE_LIBRARIES), no GPU: every row, what
its library exports, that every entry point is guarded, and the loader of _sidelib.py as the
row's binding uses it.  What is particular to one library (its constants, what it refuses) is
in that library's own test file."""
import importlib
import os
import re

import pytest

from flypylib_amd import _sidelib
from flypylib_amd.csrc import build
from tests import side_abi_cases as abi

# key -> (its row, how many names its library exports, the names)
EXPORTS = {
    'batch': (('batch', 'batchgen', 'fplb', 'fplbatch.h', 'libfplbatch.so'), 4,
              {'fplb_last_error', 'fplb_abi_version', 'fplb_struct_sizes', 'fplb_gather'}),
    'mine': (('mine', 'mine', 'fplm', 'fplmine.h', 'libfplmine.so'), 5,
             {'fplm_last_error', 'fplm_abi_version', 'fplm_voxel_loss', 'fplm_candidates_count',
              'fplm_candidates_fill'}),
    'labels': (('labels', 'labels', 'fpll', 'fpllabels.h', 'libfpllabels.so'), 3,
               {'fpll_last_error', 'fpll_abi_version', 'fpll_labels_mask'}),
    'plan': (('plan', 'plan', 'fplp', 'fplplan.h', 'libfplplan.so'), 4,
             {'fplp_last_error', 'fplp_abi_version', 'fplp_scratch_bytes', 'fplp_plan_bricks'}),
    'match': (('match', 'match', 'fple', 'fplmatch.h', 'libfplmatch.so'), 5,
              {'fple_last_error', 'fple_abi_version', 'fple_scratch_bytes', 'fple_pairs_count',
               'fple_pairs_fill'}),
    'near': (('near', 'near', 'fpln', 'fplnear.h', 'libfplnear.so'), 6,
             {'fpln_last_error', 'fpln_abi_version', 'fpln_scratch_bytes', 'fpln_cell_keys',
              'fpln_pairs_count', 'fpln_pairs_fill'}),
    'assign': (('assign', 'assign', 'fpla', 'fplassign.h', 'libfplassign.so'), 10,
               {'fpla_last_error', 'fpla_abi_version', 'fpla_scratch_bytes', 'fpla_flags_count',
                'fpla_flags_fill', 'fpla_conf_flags', 'fpla_boundaries', 'fpla_pair_costs',
                'fpla_labels', 'fpla_solve'}),
    'seg': (('seg', 'seg', 'fpls', 'fplseg.h', 'libfplseg.so'), 4,
            {'fpls_last_error', 'fpls_abi_version', 'fpls_pad_box', 'fpls_gather_labels'}),
    'merge': (('merge', 'merge', 'fplg', 'fplmerge.h', 'libfplmerge.so'), 11,
              {'fplg_last_error', 'fplg_abi_version', 'fplg_scratch_bytes', 'fplg_rows_count',
               'fplg_rows_fill', 'fplg_labels', 'fplg_group_keys', 'fplg_boundaries',
               'fplg_flags_count', 'fplg_flags_fill', 'fplg_solve'}),
    'valid': (('valid', 'valid', 'fplv', 'fplval.h', 'libfplval.so'), 3,
              {'fplv_last_error', 'fplv_abi_version', 'fplv_loss_sums'}),
    'clahe': (('clahe', 'clahe', 'fplc', 'fplclahe.h', 'libfplclahe.so'), 4,
              {'fplc_last_error', 'fplc_abi_version', 'fplc_scratch_bytes', 'fplc_clahe'}),
    'roi': (('roi', 'roi', 'fplr', 'fplroi.h', 'libfplroi.so'), 6,
            {'fplr_last_error', 'fplr_abi_version', 'fplr_mask_box', 'fplr_ptquery',
             'fplr_box_counts', 'fplr_cut_normalize_u8'}),
}
KEYS = ['batch', 'mine', 'labels', 'plan', 'match', 'near', 'assign', 'seg', 'merge', 'valid',
        'clahe', 'roi']
EAGER = ['batch', 'mine', 'labels']


def _binding(key):
    return importlib.import_module('flypylib_amd._%scapi' % key)


def _row(key):
    return next(r for r in build.SIDE_LIBRARIES if r[0] == key)


# ---- the table ---------------------------------------------------------------------------------------

def test_the_table_holds_the_twelve_rows_in_order():
    assert [r[0] for r in build.SIDE_LIBRARIES] == KEYS == list(EXPORTS)
    assert len({r[0] for r in build.SIDE_LIBRARIES}) == len({r[2] for r in build.SIDE_LIBRARIES}) == 12
    assert all(len(r) == 5 for r in build.SIDE_LIBRARIES)
    for row in build.SIDE_LIBRARIES:
        assert row[3] == {'batch': 'fplbatch.h', 'valid': 'fplval.h'}.get(row[0], 'fpl%s.h' % row[0])
        assert row[4] == 'lib' + row[3][:-2] + '.so'
    assert len({os.path.dirname(_binding(k).LIB_PATH) for k in KEYS}) == 1


def test_it_is_the_only_table_of_the_build():
    """no second table and no union of tables, under whatever name"""
    tables = [n for n, v in vars(build).items()
              if isinstance(v, tuple) and v and all(isinstance(r, tuple) for r in v)]
    assert tables == ['SIDE_LIBRARIES']
    assert [n for n in vars(build) if n.endswith(('LIBRARIES', 'LIBRARY', 'TABLES'))] == ['SIDE_LIBRARIES']
    assert build.SHARES_CSRC_HEADERS == ('seg',)


def test_three_bindings_load_eagerly():
    assert build.EAGER_BINDINGS == tuple(EAGER)
    assert _sidelib.bindings() == [_binding(k) for k in EAGER] and len(_sidelib.bindings()) == 3


@pytest.mark.parametrize('key', [k for k in KEYS if k not in EAGER])
def test_the_other_bindings_stay_lazy(key):
    assert _binding(key) not in _sidelib.bindings()


# ---- every row ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('key', KEYS)
def test_the_row_is_its_literal(key):
    row, n, names = EXPORTS[key]
    assert _row(key) == row and len(names) == n


@pytest.mark.parametrize('key', KEYS)
def test_the_library_exports_exactly_the_declared_names(key):
    _, _, prefix, header, lib = _row(key)
    if not os.path.exists(_binding(key).LIB_PATH):
        pytest.skip('%s is not built' % lib)
    assert abi.check_exports(_binding(key), header, prefix, EXPORTS[key][1]) == EXPORTS[key][2]


@pytest.mark.parametrize('key', KEYS)
def test_every_entry_point_is_guarded(key):
    _, sub, prefix, header, _ = _row(key)
    abi.check_guarded(sub, header, prefix, EXPORTS[key][1])


@pytest.mark.parametrize('key', KEYS)
def test_no_other_header_spells_the_prefix(key):
    """not in a comment either, but for fplmerge.h: its comments say whose table libfplmerge.so reads"""
    _, _, prefix, header, _ = _row(key)
    for hdr in os.listdir(os.path.join(abi.ROOT, 'include')):
        if hdr != header:
            text = open(os.path.join(abi.ROOT, 'include', hdr)).read()
            if (prefix, hdr) == ('fpln', 'fplmerge.h'):
                text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
            assert prefix + '_' not in text, hdr


@pytest.mark.parametrize('key', KEYS)
def test_the_binding_reads_its_row(key):
    _, _, prefix, _, lib = _row(key)
    side = _binding(key)._side
    assert os.path.basename(_binding(key).LIB_PATH) == lib == side.name and side.prefix == prefix
    assert side.path == _binding(key).LIB_PATH and side.signatures is _binding(key).SIGNATURES


@pytest.mark.parametrize('key', KEYS)
def test_the_library_is_loaded_once_at_the_bindings_abi(key):
    binding = _binding(key)
    lib = binding.load_library()
    assert lib is binding.load_library()
    assert getattr(lib, _row(key)[2] + '_abi_version')() == binding.ABI_VERSION


@pytest.mark.parametrize('key', KEYS)
def test_every_declared_symbol_is_bound(key):
    binding = _binding(key)
    lib = binding.load_library()
    assert set(binding.SIGNATURES) == EXPORTS[key][2]
    for name, (res, args) in binding.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


@pytest.mark.parametrize('key', KEYS)
def test_a_missing_library_is_the_bindings_own_error(key):
    binding = _binding(key)
    error = binding._side.error
    assert issubclass(error, RuntimeError) and error.__bases__ == (RuntimeError,)
    assert error.__module__ == binding.__name__
    with pytest.raises(error) as e:
        binding.load_library('/nonexistent/x.so')
    text = str(e.value)
    assert text.startswith('%s not found at /nonexistent/x.so' % _row(key)[4])
    assert 'python -m flypylib_amd.csrc.build' in text and 'no host fallback' in text
