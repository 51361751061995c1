"""The fused and cooperative pass kernels -- Chain: k_pass / k_chain_hvp (promp_kernels_pass.h, promp_kernels_chain.h); CoopFp32:
k_wide_fwd_bwd / k_wide_hvp (promp_kernels_policy_wide.h); CoopSplit: k_wb_fwd_bwd / k_wb_hvp (promp_kernels_wide_bf16.h) -- on work
items of SEVERAL rounds, shared by test_gpu_fused_rows.py (MI355X) and test_emu_fused_rows.py (emulator, a small subset).  What
tests/layered_checks.py does for the layer-by-layer family, for the three families that carry every BASELINE config.

Why: promp_plan.h's build_step_tables deals one workgroup per compute unit, capped at one per 16-row tile, and cuts the chain kernels'
rounds of four tiles into one share per compute unit.  On 256 compute units the small batches of the other test files make a work
item one tile (a chain wave one or two tiles, a workgroup one segment), so the loops of these kernels hardly ever take a second trip
on hardware:
    k_wide_*    `for (base = row_begin; base < row_end; base += R)`, R = 64 rows (fwd/bwd) and 32 (R-operator pass)
    k_wb_*      the same rounds with the most state from round to round: double-buffered observation tiles picked by `rix & 1`,
                observations requested two rounds ahead (base + 2 R), a redo that requests the first two rounds again
    k_pass / k_chain_hvp
                a wave's tiles w, w + 4, ... of a segment (the pipelined continuation pass_tile<..., true> with the pending hidden_0
                product carried across tiles, pass_flush_pending), a workgroup's segments one after the other (another task's
                parameters, distribution and observation scale restaged, accumulators and the redo state zeroed, another partial
                row), segments with tile0 > 0, the primal cache's blocks of later tiles written (k_pass<STORE>) and read
                (k_chain_hvp<CACHED>)
What a second trip can get wrong is a hardware matter -- a barrier missing between rounds, an LDS tile reused while another wave
still reads it, a register prefetch consumed a round late -- which the emulator's thread-per-lane interpreter does not judge.
PROMP_MAX_CUS plans the tables for one or two compute units; tests/host/plan_check.cpp (check_fused_row_cases) pins the tables of
every row case below -- items, segments, workgroup offsets -- and the family of every shape, and `long_items` reads the
compute-unit figure back from a context.

Comparisons and tolerances are parity_checks' own (check_loss_grad with the mean-KL objective as well, check_hvp, check_meta,
check_primal_cache, check_dice_path_lengths, check_split_range): the float64 oracle, rtol 1e-4 / atol 1e-6 on loss and KL, 1e-4 of
the max-norm on gradients and products.  Every check prints its worst figures (profiles/fused_rows.txt keeps a run's).
"""
import os

import numpy as np

from oracle import policy as op
from promp_amd import _lib
from tests import helpers, layered_checks as lc, parity_checks as pc
from tests.layered_checks import long_items, report, run_check       # noqa: F401  (the test files take them from here)

# ---- row cases: path lengths per task and the compute units to plan for.  Table 0 items (rows) | chain segments (task: tiles)
ROW_CASES = {
    # 16, 17, 65, 80 | one workgroup: t0 [0,+1) t1 [0,+2) t2 [0,+5) t3 [0,+5).  Chain: waves with no tile in a segment, a wave whose
    # second tile holds one row.  Cooperative: a third k_wb / k_wide_hvp round of one row (both observation buffers, the request two
    # rounds ahead), a second k_wide_fwd_bwd round of one row
    'A': dict(lengths=[[16], [17], [64, 1], [80]], max_cus=1),
    # 255, 256, 257 | one workgroup: 16, 16, 17 tiles.  Chain: four and five tiles per wave.  k_wide_fwd_bwd: 3 rounds + 63 rows,
    # exactly 4 rounds, 4 rounds + 1 row
    'B': dict(lengths=[[200, 55], [256], [256, 1]], max_cus=1),
    # 321, 1, 130 | one workgroup: 21, 1, 9 tiles.  A one-row task between long ones: accumulators, LDS tiles and the cotangent scale
    # left by a 21-tile segment must not leak into it
    'C': dict(lengths=[[300, 21], [1], [130]], max_cus=1),
    # 100, 100, 100 | {t0 [0,+7) t1 [0,+4)} {t1 [4,+3) t2 [0,+7)}.  A task split between two workgroups at tile 4: two partial rows
    # summed by k_reduce_task, a segment with tile0 != 0, cache blocks at a tile offset, workgroups that change task mid-launch
    'D': dict(lengths=[[100], [100], [100]], max_cus=2),
    # [0, 256) [256, 513) | {t0 [0,+20)} {t0 [20,+13)}.  tile0 = 20; cooperative items that begin 256 rows into a task
    'E': dict(lengths=[[513]], max_cus=2),
}

# ---- shapes: one per instantiation of the three families.  `family`, `padded`: what promp_plan.h's pass_family / pad_dims give
#      (asserted by shape_kwargs through tests/helpers.py, pinned against the C++ by tests/host/plan_check.cpp)
ROW_SHAPES = {
    # Chain: k_pass / k_chain_hvp <NC1, NC2, observation k-steps>
    'h32x32_o7_a3': dict(hidden=(32, 32), O=7, A=3, family='Chain'),                            # 2 k-steps
    'h32x64_o20_a6': dict(hidden=(32, 64), O=20, A=6, family='Chain'),                          # 5 k-steps
    'h64x32_o29_a8': dict(hidden=(64, 32), O=29, A=8, family='Chain'),                          # 8 k-steps, every action slot owned
    'h64x64_o32_a1': dict(hidden=(64, 64), O=32, A=1, family='Chain'),                          # every second action slot unowned
    'h48x20_o11_a7': dict(hidden=(48, 20), O=11, A=7, family='Chain', padded=(64, 32)),         # zero-padded, odd act_dim
    # CoopFp32: k_wide_* <width, NOB>
    'h64x64_o33_a3': dict(hidden=(64, 64), O=33, A=3, family='CoopFp32'),                       # NOB 4, one observation past NOB 2
    'h64x64_o64_a5': dict(hidden=(64, 64), O=64, A=5, family='CoopFp32'),                       # NOB 4, full
    'h64x64_o111_a8': dict(hidden=(64, 64), O=111, A=8, family='CoopFp32'),                     # NOB 8
    'h128x128_o128_a8': dict(hidden=(128, 128), O=128, A=8, family='CoopFp32'),                 # k_wide<128, 8>
    'h48x20_o40_a3': dict(hidden=(48, 20), O=40, A=3, family='CoopFp32', padded=(64, 64)),      # zero-padded
    # CoopSplit: k_wb_* by observation class
    'h128x128_o20_a8': dict(hidden=(128, 128), O=20, A=8, family='CoopSplit'),                  # class 1, eight actions
    'h128x128_o111_a8': dict(hidden=(128, 128), O=111, A=8, family='CoopSplit'),                # class 2
    'h128x128_o127_a1': dict(hidden=(128, 128), O=127, A=1, family='CoopSplit'),                # class 3, one action
    'h100x100_o50_a4': dict(hidden=(100, 100), O=50, A=4, family='CoopSplit', padded=(128, 128)),   # zero-padded
}
# k_wide<128, 2>: (128,128) at obs 20 is CoopSplit's unless PROMP_WIDE_FP32=1 keeps it on the exact-FP32 kernels
SWITCHED_SHAPES = {
    'h128x128_o20_a6_fp32': dict(hidden=(128, 128), O=20, A=6, family='CoopFp32', wide_fp32=True),
}
ALL_SHAPES = dict(ROW_SHAPES, **SWITCHED_SHAPES)
FAMILY_SHAPES = {f: [n for n, s in ROW_SHAPES.items() if s['family'] == f] for f in ('Chain', 'CoopFp32', 'CoopSplit')}
ONE_PER_FAMILY = ['h32x64_o20_a6', 'h64x64_o33_a3', 'h128x128_o20_a8']
META_CASES = ['B', 'D', 'E']         # check_meta and check_primal_cache: several rounds, two partial rows, tile0 = 20

# seeds under which the inputs meet dropped_row_sensitivity's condition, per shape for the cases A, B, C, D, E: for each pair the
# first seed from 900 on that does (with eight actions and 250+ rows the PPO clip sits on the longest task's last row under most
# seeds: no gradient from that row under 'clip')
_SEEDS = {
    'h32x32_o7_a3': (900, 900, 900, 900, 902), 'h32x64_o20_a6': (900, 902, 903, 900, 902), 'h64x32_o29_a8': (901, 900, 902, 901, 900),
    'h64x64_o32_a1': (900, 900, 900, 900, 900), 'h48x20_o11_a7': (901, 900, 900, 900, 901),
    'h64x64_o33_a3': (900, 900, 900, 901, 901), 'h64x64_o64_a5': (900, 902, 903, 901, 901), 'h64x64_o111_a8': (907, 902, 906, 905, 900),
    'h128x128_o128_a8': (902, 907, 926, 900, 903), 'h48x20_o40_a3': (904, 902, 901, 901, 900),
    'h128x128_o20_a6_fp32': (903, 902, 903, 915, 901),
    'h128x128_o20_a8': (901, 909, 911, 900, 905), 'h128x128_o111_a8': (913, 906, 914, 901, 903), 'h128x128_o127_a1': (900, 900, 901, 900, 900),
    'h100x100_o50_a4': (902, 900, 900, 902, 901),
}
ROW_SEEDS = {(case, shape): seeds[i] for shape, seeds in _SEEDS.items() for i, case in enumerate('ABCDE')}
ROW_PAIRS = [(case, shape) for shape in ALL_SHAPES for case in sorted(ROW_CASES)]       # every GPU case


def family_of(O, A, hidden, wide_fp32=False):
    """promp_plan.h pad_dims + pass_family for a shape on the fused kernels -> (family, padded widths)"""
    assert not helpers.runs_layer_by_layer(O, A, hidden), (hidden, O, A)
    padded = helpers.padded_hidden(O, A, hidden)
    if O <= 32 and padded[0] != 128:
        return 'Chain', padded
    if padded[0] == 128 and O <= 127 and not wide_fp32:
        return 'CoopSplit', padded
    return 'CoopFp32', padded


def wide_fp32_is_set():
    return int(os.environ.get('PROMP_WIDE_FP32') or 0) != 0        # promp_plan.h: plan_switches_from_env


def shape_kwargs(lengths, hidden, O, A, family, padded=None, wide_fp32=False, **_):
    """the arguments of parity_checks' comparisons for one shape on explicit path lengths; `family` (and `padded`, where the widths
    are not instantiated themselves): where the shape is meant to run -- a dispatch that has moved it, or a switch that is not as
    the shape wants it, fails here instead of quietly testing another family"""
    assert wide_fp32_is_set() == bool(wide_fp32), 'PROMP_WIDE_FP32 is %s' % os.environ.get('PROMP_WIDE_FP32')
    assert family_of(O, A, hidden, wide_fp32) == (family, tuple(padded or hidden)), (hidden, O, A, family_of(O, A, hidden, wide_fp32))
    return dict(M=len(lengths), P=None, T=None, O=O, A=A, hidden=tuple(hidden), lengths_per_task=lengths)


def plan(monkeypatch, lib, max_cus, shape=None):
    """long_items for a shape of ALL_SHAPES: PROMP_MAX_CUS, and PROMP_WIDE_FP32 as the shape wants it (cleared for every other)"""
    long_items(monkeypatch, lib, max_cus, wide_fp32=bool(shape and ALL_SHAPES[shape].get('wide_fp32')))


# ---- a condition on the INPUTS (oracle alone, no kernel): a dropped row must show
def last_row_sensitivity(case, shape):
    s = ALL_SHAPES[shape]
    return lc.dropped_row_sensitivity(tuple(map(tuple, ROW_CASES[case]['lengths'])), ROW_SEEDS[case, shape], s['O'], s['A'], tuple(s['hidden']))


def check_inputs_show_a_dropped_row(case, shape):
    """ten times the comparison's tolerance: if a seed does not give it, ROW_SEEDS takes another seed, never a smaller bound"""
    moved = last_row_sensitivity(case, shape)
    print('fused rows %s %s: the oracle gradient of the longest task moves by %.2e of its max-norm without its last row' % (case, shape, moved))
    assert moved > 1e-3, (case, shape, moved)


def check_rows(lib, case, shape, what, tag='', **kw):
    """row case A-E at ALL_SHAPES[shape] (the caller has set the switches: plan(..., ROW_CASES[case]['max_cus'], shape));
    loss_grad runs the mean-KL objective as well"""
    check_inputs_show_a_dropped_row(case, shape)
    if what == 'loss_grad':
        kw = dict(kw, kl_objective=True)
    return run_check(lib, 'rows %s %s%s' % (case, shape, tag), what, ROW_SEEDS[case, shape],
                     shape_kwargs(ROW_CASES[case]['lengths'], **ALL_SHAPES[shape]), family='fused', **kw)


def check_cache(lib, case, shape):
    """check_primal_cache on a row case: k_pass<STORE> writes and k_chain_hvp<CACHED> reads the cache blocks of a wave's later tiles
    and of segments with tile0 > 0"""
    check_inputs_show_a_dropped_row(case, shape)
    worst = {}
    kw = shape_kwargs(ROW_CASES[case]['lengths'], **ALL_SHAPES[shape])
    try:
        pc.check_primal_cache(lib, ROW_SEEDS[case, shape], K=1, worst=worst, **kw)
    finally:
        report('rows %s %s primal_cache' % (case, shape), worst, 'fused')
    return worst


# ---- DICE-MAML: the row tangents of a path are written across tiles / rounds and read back by k_dice_scan
DICE_LENGTHS = lc.DICE_LENGTHS                  # 321 and 194 rows, one work item each at one compute unit
DICE_SHAPES = {
    'h32x64_o9_a3': dict(hidden=(32, 64), O=9, A=3, family='Chain'),
    'h64x64_o40_a3': dict(hidden=(64, 64), O=40, A=3, family='CoopFp32'),
    'h72x40_o9_a3': dict(hidden=(72, 40), O=9, A=3, family='CoopSplit', padded=(128, 128)),
}


def check_dice(lib, shape):
    s = DICE_SHAPES[shape]
    shape_kwargs(DICE_LENGTHS, **s)
    worst = {}
    try:
        pc.check_dice_path_lengths(lib, 711, DICE_LENGTHS, O=s['O'], A=s['A'], hidden=s['hidden'], worst=worst)
    finally:
        report('dice %s %s' % (shape, DICE_LENGTHS), worst, 'fused')
    return worst


# ---- the FP16 split's range on one compute unit: M = 2 tasks of 2 x 160 rows, one work item / one 20-tile segment each.  Chain: one
#      workgroup walks both segments and the heavy-tailed case has to walk the SECOND again as well (k_pass: `sg -= 1` behind a
#      finished segment, `attempt = 0` in front of the next)
RANGE_SHAPES = {
    'h64x64_o20_a6': dict(hidden=(64, 64), O=20, A=6, family='Chain'),
    'h128x128_o20_a6': dict(hidden=(128, 128), O=20, A=6, family='CoopSplit'),
}


def check_range(lib, shape):
    """parity_checks.check_split_range as tests/test_gpu_parity.py runs it at these two shapes (its tolerance 2.5e-6)"""
    s = RANGE_SHAPES[shape]
    shape_kwargs([[160, 160]] * 2, **s)
    pc.check_split_range(lib, s['hidden'], s['O'], s['A'], M=2, P=2, T=160, tol=2.5e-6, min_pass_redo=2 if s['family'] == 'Chain' else 0)


# ---- a switch that is ignored would repeat the default family: the two round differently, never to the same bits
def gradients(lib, case, shape):
    """eval_loss_grad's ratio gradient of row case `case` at ALL_SHAPES[shape], under the switches as they are now"""
    s = ALL_SHAPES[shape]
    lengths, seed = ROW_CASES[case]['lengths'], ROW_SEEDS[case, shape]
    theta, all_slabs, all_paths = helpers.make_promp_case(seed, len(lengths), None, None, s['O'], s['A'], s['hidden'], 1, lengths_per_task=lengths)
    assert theta.size == op.PolicySpec(s['O'], s['A'], s['hidden']).n_params
    ctx = pc.make_ctx(lib, len(lengths), s['O'], s['A'], s['hidden'], 1, all_paths)
    try:
        helpers.upload_slabs(ctx, all_paths, all_slabs)
        ctx.set_task_thetas(np.tile(theta, (len(lengths), 1)))
        return ctx.eval_loss_grad(1, _lib.LOSS_RATIO)[0]
    finally:
        ctx.close()


# ---- emulator subset: one launch set over at most 321 rows
EMU_CASES = {
    # row case D on two units: a task split between two workgroups at tile 4
    'D_h32x32_o7_a3': dict(lengths=ROW_CASES['D']['lengths'], max_cus=2, seed=ROW_SEEDS['D', 'h32x32_o7_a3'], shape=ROW_SHAPES['h32x32_o7_a3']),
    # one item of 65 rows: a second 64-row round and a third 32-row round of one row
    'rows65_h64x64_o40_a3': dict(lengths=[[64, 1]], max_cus=1, seed=731, shape=DICE_SHAPES['h64x64_o40_a3']),
}


def check_emu(lib, name, what):
    c = EMU_CASES[name]
    return run_check(lib, 'emu %s' % name, what, c['seed'], shape_kwargs(c['lengths'], **c['shape']), family='fused',
                     **(dict(kl_objective=True) if what == 'loss_grad' else {}))
