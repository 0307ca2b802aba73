"""CPU: the op plan of the fp32 MFMA executor (csrc/mfma_f32_plan.h), built alone with the host C++
compiler.  The plan accepts the programs, and states the launches, that the rules conv_mfma_f32.hip
carried inline before the header existed did - restated in tests/mfma_f32_cases.py - on every case
of the executor's test tables and on a seeded sweep of random programs; the only programs it newly
declines are those the old launch loop refused with an error after the dispatcher had picked it.
Its fragment offsets are the old packing and launch arithmetic, restated here."""
import collections
import os
import re

import pytest

from flypylib_amd.program import LayerGraph
from tests import deconv_cases, dilated_cases, down_cases, mfma_f32_cases as mc, mfma_f32_plan_cases as pc

CSRC = os.path.join(pc.ROOT, 'flypylib_amd', 'csrc')

# the classes of programs the old acceptance rule took and the old launch loop then refused, by the
# error of that time (mfma_f32_cases.launch_refusal) -> the reasons the plan gives for declining them
REFUSAL_CLASSES = {
    'add of incompatible tensors': {'add of incompatible tensors'},       # an add of an up(2) view or of a virtual concatenation
    'unsupported concat': {'unsupported concat'},                         # a conv3 of a concatenation of a concatenation
}


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    exe = pc.build_driver(tmp_path_factory.mktemp('mfma_f32_plan'))
    if not exe:
        pytest.skip('no host C++ compiler')
    return exe


def _both(driver, programs):
    """[(plan fused, plan unfused)] of (ops, out_tensor) programs"""
    plans, _ = pc.ask_plans(driver, [(o, t, u) for o, t in programs for u in (False, True)])
    return list(zip(plans[0::2], plans[1::2]))


def _lowered(graph):
    ops, _, out_tensor, _ = graph.lower_inference()
    return ops, out_tensor


def _table_programs():
    """{name: (ops, out_tensor)}: every case of the executor's tables, at its smallest tile"""
    out = {}
    for kind, cin, cout, v in mc.CONV_CASES + [mc.SIGMOID_CASE]:
        tile = mc.SIGMOID_TILE if v == 'sigmoid' else mc.tiles_of(kind, cin, cout)[0]
        out['conv %s %d %d %s' % (kind, cin, cout, v)] = _lowered(mc.conv_case(kind, cin, cout, v, tile)['graph'])
    for kind, cin, cout, tile, _ in mc.TAP_CASES:
        out['tap %s %d %d' % (kind, cin, cout)] = _lowered(mc.tap_case(kind, cin, cout, tile)[0])
    for case in mc.FUSED_CASES + mc.UNFUSED_CASES + mc.STEM_FUSED_CASES + mc.STEM_UNFUSED_CASES:
        out['chain %r' % (case,)] = _lowered(mc.fused_case(*case, tile=7)['graph'])
    for name in mc.EXACT_CASES:
        out['exact ' + name] = _lowered(mc.exact_case(name)['graph'])
    for kind, cin, cout, tile, lifts in mc.DECLINED_CASES + mc.NEIGHBOUR_CASES:
        out['edge %s %d %d %r' % (kind, cin, cout, lifts)] = _lowered(mc.conv_case(kind, cin, cout, 'bias', tile, lifts)['graph'])
    out['tiny_unet_t'] = _lowered(deconv_cases.tiny_unet_t()[0])
    out['tiny_vnet'] = _lowered(down_cases.tiny_vnet()[0])
    out['tiny_atrous'] = _lowered(dilated_cases.tiny_atrous()[0])
    for cin, cout in ((1, 8), (16, 16), (40, 130), (256, 256)):
        out['deconv %d %d' % (cin, cout)] = _lowered(deconv_cases.deconv_graph(cin, cout, True, True, False, (4, 4, 4))[0])
        out['down %d %d' % (cin, cout)] = _lowered(down_cases.down_graph(cin, cout, True, True, False, (4, 4, 4))[0])
    for cin, cout in ((1, 8), (16, 65), (40, 130), (192, 256)):
        out['dilated %d %d' % (cin, cout)] = _lowered(dilated_cases.dilated_graph(cin, cout, True, True, False, (6, 6, 6))[0])
    return out


def test_header_holds_the_limits_and_the_executor_none_of_them(driver):
    _, consts = pc.ask_plans(driver, [])
    assert consts == dict(MB_MAX=4, SLICE=64, CONV3_COUT_MAX=256, SLICES_MAX=4, CONV3_CHUNKS_MAX=12, GEMM2_C_MAX=256,
                          CONV1_MB=[1, 2, 3, 4, 6, 8], FUSED_MB=[2, 3, 4], STEM_FUSED_MB=[2, 3])
    text = open(os.path.join(CSRC, 'conv_mfma_f32.hip')).read()
    host = text[text.index('bool fpl_mfma_f32_supported'):text.index('Training-side entry points')]
    assert '#include "mfma_f32_plan.h"' in text
    assert 'bool fpl_mfma_f32_supported(const fpl_program *prog) { return plan_of(prog).ok; }' in host
    for moved in ('concats_written', 'readers(', 'is_view', 'pair_ok', '12 * 16', '> 256', '> 64', '* 256', 'c0 += 64',
                  'kind == FPL_OP_CONCAT'):
        assert moved not in host, moved
    assert len(re.findall(r'getenv\("FPL_F32_UNFUSED"\)', text)) == 1
    assert 'getenv' not in open(os.path.join(CSRC, 'mfma_f32_plan.h')).read().split('#pragma once')[1]


def test_every_table_case_plans_as_the_restated_rules_say(driver):
    table = _table_programs()
    forms = collections.Counter()
    for (name, (ops, out_tensor)), (fused, unfused) in zip(table.items(), _both(driver, table.values())):
        sup = mc.supported_ops(ops, out_tensor)
        assert mc.launch_refusal(ops, out_tensor) is None or not sup, name
        for plan, flag in ((fused, False), (unfused, True)):
            assert plan['ok'] == sup, (name, plan['reason'])
            want = mc.predict_launches_ops(ops, out_tensor, unfused=flag)
            assert (pc.plan_launches(plan) if plan['ok'] else None) == want, (name, flag, plan, want)
        assert fused['frag_floats'] == unfused['frag_floats']
        forms.update(s['form'] for p in (fused, unfused) for s in p['steps'])
        if name.startswith('edge'):
            assert (fused['bad_op'] >= 0) == (not sup) and bool(fused['reason']) == (not sup)
    # the tables reach every form but the written concatenation of a network that reads it with a
    # 1x1x1 conv: tiny_unet_t
    assert set(forms) == set(pc.LAUNCH_NAME), forms
    unet = dict(zip(table, _both(driver, table.values())))['tiny_unet_t'][0]
    assert [s['form'] for s in unet['steps']].count('concat') == 1
    # tiles that are not cubic: programs of voxel GEMMs and dilated convs, but not of 1x1x1 convs alone
    plans = dict(zip(table, _both(driver, table.values())))
    assert plans['deconv 16 16'][0]['takes_other'] == 1 and plans['dilated 16 65'][0]['takes_other'] == 1
    assert plans['down 1 8'][0]['any_dims'] == 1 and plans['down 1 8'][0]['takes_other'] == 1
    lift = plans['conv conv1 1 48 none'][0]
    assert lift['any_dims'] == 1 and lift['takes_other'] == 0 and lift['takes_cubic'] == 1
    assert plans['tiny_unet_t'][0]['any_dims'] == 0 and plans['tiny_unet_t'][0]['takes_other'] == 0


def test_sweep_of_random_programs(driver):
    programs = pc.sweep()
    assert len(programs) == 2000 and all(2 <= len(o) <= 8 for o, _ in programs)
    assert {o['kind'] for ops, _ in programs for o in ops} == set(range(9))
    accepted = declined = moved = 0
    in_form, classes = collections.Counter(), collections.Counter()
    for (ops, out_tensor), (fused, unfused) in zip(programs, _both(driver, programs)):
        assert fused['ok'] == unfused['ok'] and fused['frag_floats'] == unfused['frag_floats']
        if not mc.supported_ops(ops, out_tensor):
            declined += 1
            assert not fused['ok'], (ops, fused)
            continue
        refusal = mc.launch_refusal(ops, out_tensor)
        if refusal is not None:
            # accepted then, and refused at launch with this error: declined now
            assert not fused['ok'] and fused['reason'] in REFUSAL_CLASSES[refusal], (ops, refusal, fused)
            classes[refusal] += 1
            moved += 1
            continue
        accepted += 1
        for plan, flag in ((fused, False), (unfused, True)):
            assert plan['ok'], (ops, plan['bad_op'], plan['reason'])
            assert pc.plan_launches(plan) == mc.predict_launches_ops(ops, out_tensor, unfused=flag), (ops, flag, plan)
        in_form.update({s['form'] for s in fused['steps']})
    print('sweep: %d run as before, %d declined as before, %d declined now (refused at launch before): %s'
          % (accepted, declined, moved, dict(classes)))
    print('programs per form:', dict(in_form))
    assert accepted >= 500 and declined >= 500
    assert set(in_form) == set(pc.LAUNCH_NAME) and min(in_form.values()) >= 20, in_form
    assert moved < 0.05 * len(programs)


def _lift(dst, c, src=0):
    return pc._op(0, src, dst, 1, c, k=1)


# the smallest program of each class that the old rule accepted and the old launch loop refused
MOVED_PROGRAMS = {
    'add of an up-sampled view': ('add of incompatible tensors', [
        _lift(1, 16), pc._op(2, 1, 2, 16, 16, p=(2, 2, 2, 0, 0, 0)), _lift(3, 16), pc._op(5, 2, 4, 16, 16, src1=3)]),
    'add of a virtual concatenation': ('add of incompatible tensors', [
        _lift(1, 16), _lift(2, 16), pc._op(4, 1, 3, 16, 32, src1=2), _lift(4, 32), pc._op(5, 3, 5, 32, 32, src1=4)]),
    'conv3 of a concatenation of a concatenation': ('unsupported concat', [
        _lift(1, 16), pc._op(4, 1, 2, 16, 32, src1=1), pc._op(4, 2, 3, 32, 48, src1=1), pc._op(0, 3, 4, 48, 16, k=3)]),
}


@pytest.mark.parametrize('name', sorted(MOVED_PROGRAMS))
def test_programs_refused_at_launch_before_are_declined_now(driver, name):
    error, ops = MOVED_PROGRAMS[name]
    out_tensor = ops[-1]['dst']
    assert mc.supported_ops(ops, out_tensor) and mc.launch_refusal(ops, out_tensor) == error
    (fused, unfused), = _both(driver, [(ops, out_tensor)])
    for plan in (fused, unfused):
        assert not plan['ok'] and plan['bad_op'] == len(ops) - 1 and plan['reason'] in REFUSAL_CLASSES[error]
        assert plan['steps'] == [] and plan['takes_cubic'] == 0


# ---- fragment layout --------------------------------------------------------------------------
def _b16(c):
    return (c + 15) // 16


def _old_layout(ops):
    """per conv-like op, in op order: (length, slice offsets inside it, shift offset inside it) in floats,
    from the pack_*_f32 functions' `assign` sizes and the launch loop's pointer arithmetic as they were"""
    out = []
    for o in ops:
        cin, cout, mb = o['cin'], o['cout'], _b16(o['cout'])
        if o['kind'] == 6:
            nkb, nb2 = _b16(cin), _b16(2 * cout)
            out.append((4 * nb2 * nkb * 256 + 16 * nb2, [], 4 * nb2 * nkb * 256))
        elif o['kind'] == 7:
            nkb = _b16(2 * cin)
            nbt = 2 if nkb <= 2 else 4
            nbp = (mb + nbt - 1) // nbt * nbt
            out.append((4 * nkb * nbp * 256 + 16 * nbp, [], 4 * nkb * nbp * 256))
        elif o['kind'] == 8 or (o['kind'] == 0 and o['k'] == 3 and cin > 1):
            offs, woff = [], 0
            for c0 in range(0, cout, 64):
                offs.append(woff)
                woff += _b16(cin) * 27 * _b16(min(64, cout - c0)) * 256
            out.append((woff, offs, 0))
        elif o['kind'] == 0 and o['k'] == 3:
            out.append((2 * mb * 256, [], 0))
        elif o['kind'] == 0:
            out.append((_b16(cin) * mb * 256, [], 0))
    return out


def _layout_graph():
    """one op of each convolution kind: stem 1 -> 32, conv1 32 -> 32 and a pool (one fused kernel), conv3
    32 -> 130 (three slices), dilated 130 -> 65 (two), deconv 65 -> 20, down 20 -> 24 (any-cin form: 40
    K values per tap pair), conv1 24 -> 5, down 5 -> 9 (one K-block in registers), down 9 -> 7 (two)"""
    g = LayerGraph((40, 40, 40))
    n = g.pool(g.conv(g.conv(g.input(), 32, 3, activation='relu'), 32, 1, activation='relu'))
    n = g.dilated(g.conv(n, 130, 3), 65)
    n = g.conv(g.down(g.deconv(n, 20), 24), 5, 1)
    g.finish(g.down(g.down(n, 9), 7))
    return g


def test_fragment_layout_is_the_old_packing_and_launch_arithmetic(driver):
    ops, out_tensor = _lowered(_layout_graph())
    (fused, unfused), = _both(driver, [(ops, out_tensor)])
    assert [s['form'] for s in fused['steps']] == ['stem_conv1_pool', 'conv3', 'atrous', 'deconv', 'down', 'conv1',
                                                   'down', 'down']
    assert [s['form'] for s in unfused['steps']][:3] == ['stem', 'conv1', 'pool']
    old = _old_layout(ops)
    assert len(old) == 9 and [len(b[1]) for b in old] == [0, 0, 3, 2, 0, 0, 0, 0, 0]
    starts, total = [], 0
    for length, _, _ in old:
        starts.append(total)
        total += length
    for plan in (fused, unfused):
        assert plan['frag_floats'] == total
        blocks = {}                                           # op -> (offset, length, slice offsets, shift offset)
        end = 0
        for s in plan['steps']:
            assert s['frag_off'] == end                       # no gap, no overlap, in launch order
            end += s['frag_len']
            conv = [i for i in s['ops'] if ops[i]['kind'] != 1]
            if not conv:
                assert s['frag_len'] == 0
                continue
            first_len = (s['frag1_off'] - s['frag_off']) if s['mb1'] else s['frag_len']
            blocks[conv[0]] = (s['frag_off'], first_len, [sl[3] - s['frag_off'] for sl in s['slices']], s['shift_off'])
            if s['mb1']:
                blocks[conv[1]] = (s['frag1_off'], s['frag_off'] + s['frag_len'] - s['frag1_off'], [], 0)
        assert end == total
        conv_ops = [i for i, o in enumerate(ops) if o['kind'] in (0, 6, 7, 8)]
        assert sorted(blocks) == conv_ops
        for i, start, (length, offs, shift) in zip(conv_ops, starts, old):
            assert blocks[i] == (start, length, offs, shift), (i, ops[i], blocks[i], (start, length, offs, shift))
    # the slices themselves
    conv3 = fused['steps'][1]
    assert [sl[:3] for sl in conv3['slices']] == [[0, 64, 4], [64, 64, 4], [128, 2, 1]]
    assert [sl[:3] for sl in fused['steps'][2]['slices']] == [[0, 64, 4], [64, 1, 1]]
    assert (fused['steps'][0]['mb'], fused['steps'][0]['mb1'], fused['steps'][0]['pool']) == (2, 2, 1)
