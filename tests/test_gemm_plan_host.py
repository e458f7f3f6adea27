"""The GEMM launch plan, host side (no GPU): rmem_conv_plan -- the function rmem_conv2d_nhwc, rmem_conv1x1_dual_nhwc,
rmem_linear_grouped and rmem_conv_workspace_bytes take their decision from -- against the Python restatement of the dispatch
rules (tests/gemm_plan_ref.py), on the shapes the GPU tests and the scripts run; and that those GPU tests reach every kernel
instantiation gemm_conv.hip builds."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import gemm_plan_ref as R
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import gemm_bench  # noqa: E402
import pc_check  # noqa: E402
import test_hip_ops as G  # noqa: E402


def conv(H, W, Cin, Cout, k=1, stride=1, pad=0, batch=1, entry=R.CONV2D, extra=0):
    return dict(H=H, W=W, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, batch=batch, entry=entry, extra=extra)


def dual(B, H2, W2, K1, K2, Cout, stride):
    return conv((H2 - 1) // stride + 1, (W2 - 1) // stride + 1, K1, Cout, batch=B, entry=R.DUAL, extra=K2)


# the shapes the GPU tests run.  test_conv2d launches each of CONV_SHAPES without and with the split-K workspace; nothing else
# passes one
CONV_SHAPES = [conv(*c[:7]) for c in dict.fromkeys(G.CONV_CASES)]
DUAL_SHAPES = [dual(*c) for c in G.DUAL_CASES]
_grouped = [G.GROUPED_LAUNCH] + G.GROUPED_CASES                # each as one grouped launch and as single launches
GROUPED_SHAPES = ([conv(M, 1, K, N, entry=R.LINEAR_GROUPED, extra=n) for M, K, N, n in _grouped]
                  + [conv(M, 1, K, N) for M, K, N, n in _grouped])
PC_SHAPES = [conv(H, W, ci, co, k, st, k // 2, B) for B, H, W, ci, co, k, st, _ in pc_check.CONV_SHAPES]
# scripts/gemm_bench.py at its default 16 images / 8 clips per launch (no GPU test runs these: they do not count as coverage)
BENCH_SHAPES = [conv(1674 * 8 if H == 6696 else H, W, ci, co, k, st, k // 2, {8: 16, 4: 8, 1: 1}[b]) for H, W, ci, co, k, st, b in gemm_bench.SHAPES]
GPU_SHAPES = CONV_SHAPES + DUAL_SHAPES + GROUPED_SHAPES + PC_SHAPES


@pytest.fixture(scope='module')
def lib():
    from rmem_ocu_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def lib_plan(s, has_ws):
    from rmem_ocu_amd import _lib, ops
    return ops.conv_plan(H=s['H'], W=s['W'], Cin=s['Cin'], Cout=s['Cout'], KH=s['k'], KW=s['k'], stride=s['stride'], pad=s['pad'],
                         batch=s['batch'], has_ws=has_ws, entry=_lib.GEMM_ENTRIES[s['entry']], extra=s['extra'])


def ref_plan(s, has_ws, pc=2):
    return R.plan(has_ws=has_ws and s['entry'] == R.CONV2D, pc=pc, **s)


def test_restatement_agrees_with_rows_derived_by_hand():
    """Rows worked out by hand from the dispatcher this plan replaced."""
    F = R.FAMILY_NAMES.index

    def check(s, ws, **want):
        p = ref_plan(s, ws)
        assert {k: p[k] for k in want} == want, (s, ws, p)

    l3 = conv(31, 54, 256, 256, 3, 1, 1)                      # M 1674, K 2304: 36 k-steps on 108 tiles
    check(l3, True, family=F('general64'), splits=5, steps_per_split=8, grid_x=27, grid_y=4, grid_z=5, xcd_ny=0, ring=1)
    check(l3, False, family=F('scalar64'), ring=3, splits=1, xcd_ny=4, grid_x=128, grid_y=1, grid_z=1)
    for ws in (False, True):
        check(conv(1674, 1, 1024, 256), ws, family=F('scalar64'), ring=3, splits=1, xcd_ny=4, grid_x=128)      # 16 k-steps: never split
        check(conv(61, 107, 512, 128, batch=16), ws, family=F('pc128'), ring=2, threads=512, grid_x=816, grid_y=1, grid_z=1, xcd_ny=0)
        check(conv(97, 129, 8, 64, 7, 2, 3), ws, family=F('rowrun64'), ring=3, grid_x=50, grid_y=1, grid_z=1)
        check(conv(500, 1, 128, 11), ws, family=F('scalar64'), ring=1, xcd_ny=0, splits=1)
    idb = conv(481, 849, 16, 256, 17, 16, 8)                  # M 1674, K 4624: 73 k-steps
    check(idb, True, family=F('general64'), splits=5, steps_per_split=15)
    check(idb, False, family=F('rowrun128'), ring=3, grid_x=14, grid_y=2, grid_z=1, xcd_ny=0)


@pytest.mark.parametrize('has_ws', [False, True])
def test_plan_equals_restatement(lib, has_ws):
    assert os.environ.get('RMEM_GEMM_PC') is None and os.environ.get('RMEM_GEMM_FAST') is None and os.environ.get('RMEM_GEMM_XCD') is None
    for s in GPU_SHAPES + BENCH_SHAPES:
        assert lib_plan(s, has_ws) == ref_plan(s, has_ws), (s, has_ws)


def test_workspace_bytes_follow_the_plan(lib):
    from rmem_ocu_amd._lib import ConvDesc
    split = 0
    for s in CONV_SHAPES + PC_SHAPES + BENCH_SHAPES:
        Ho, Wo = R.out_size(s['H'], s['W'], s['k'], s['stride'], s['pad'])
        d = ConvDesc(s['H'], s['W'], s['Cin'], Ho, Wo, s['Cout'], s['k'], s['k'], s['stride'], s['pad'], s['Cout'], s['Cout'], s['Cout'],
                     0, 0, 0, 0, s['batch'], 0, 0, 0, 0)
        p = lib_plan(s, True)
        want = p['splits'] * s['batch'] * Ho * Wo * s['Cout'] * 4 if p['splits'] > 1 else 0
        assert lib.rmem_conv_workspace_bytes(ctypes.byref(d)) == want, s
        assert lib_plan(s, False)['splits'] == 1
        split += p['splits'] > 1
    assert split >= 4


def test_geometry_errors_need_no_pointers(lib):
    from rmem_ocu_amd import ops
    from rmem_ocu_amd._lib import RmemError
    for kw, msg in ((dict(Cin=12), 'multiple of 8'), (dict(KH=0), 'bad kernel geometry'), (dict(ldx=8), 'ldx needs'),
                    (dict(entry='conv1x1_dual', extra=32), 'multiples of 64'), (dict(entry='linear_grouped', extra=5), '1..4 problems'),
                    (dict(entry='linear_grouped', extra=2, KH=3, KW=3, pad=1), '1x1 stride-1 problems only')):
        with pytest.raises(RmemError, match=msg):
            ops.conv_plan(**{**dict(H=8, W=8, Cin=64, Cout=16), **kw})


CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import test_gemm_plan_host as T
from rmem_ocu_amd._lib import RmemError
try:
    print(json.dumps([T.lib_plan(s, False) for s in T.PC_SHAPES]))
except RmemError as e:
    print(json.dumps(str(e)))
"""


@pytest.fixture(scope='module')
def pc_children(lib):
    """The plans of the pc_check shapes under RMEM_GEMM_PC = 0, 1, 3 and 7: the knob is read once per process, so each setting gets
    a child process (host only; all four run side by side)."""
    procs = {}
    for v in ('0', '1', '3', '7'):
        env = dict(os.environ, RMEM_GEMM_PC=v)
        code = CHILD.format(paths=[os.path.join(ROOT, 'tests'), ROOT])
        procs[v] = subprocess.Popen([sys.executable, '-c', code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for v, p in procs.items():
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, se[-2000:]
        out[v] = json.loads(so.strip().splitlines()[-1])
    return out


@pytest.mark.parametrize('pc', ['0', '1', '3'])
def test_plan_equals_restatement_under_the_pc_knob(pc_children, pc):
    assert pc_children[pc] == [ref_plan(s, False, pc=int(pc)) for s in PC_SHAPES]


def test_bad_pc_knob_fails_the_call(pc_children):
    assert isinstance(pc_children['7'], str) and 'RMEM_GEMM_PC' in pc_children['7']


def test_gpu_tests_reach_every_kernel(lib, pc_children):
    """Every (family, ring, is1x1) instantiation the plan can return -- all 25 kernels gemm_conv.hip builds per element type -- is
    launched by a GPU test: test_conv2d (with and without the split-K workspace), test_conv1x1_dual_bottleneck_tail, the grouped
    tests, and scripts/pc_check.py under the three RMEM_GEMM_PC settings test_producer_consumer_forms_are_bit_identical uses."""
    got = set()
    for s in CONV_SHAPES:
        got |= R.kernels(lib_plan(s, True))
    for s in GPU_SHAPES:
        got |= R.kernels(lib_plan(s, False))
    for pc in ('0', '3'):
        for p in pc_children[pc]:
            got |= R.kernels(p)
    assert got == R.ALL_KERNELS, (sorted(R.ALL_KERNELS - got, key=str), sorted(got - R.ALL_KERNELS, key=str))
