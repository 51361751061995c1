"""The layer-by-layer kernels (promp_kernels_generic.h, promp_kernels_generic_bf16.h) on LONG work items and at the edges of their
widths, shared by test_gpu_layered.py (MI355X) and test_emu_layered.py (emulator, a small subset).

Why: work table 0 holds one workgroup per compute unit, capped at one per 16-row tile (promp_plan.h: build_step_tables).  On 256
compute units the small batches of the other test files make every work item ONE tile, so none of the row loops of these kernels
runs a second time there:
    k_gb_linear / k_gen_linear   rounds of 64 rows, dealt to GEN_SPLIT = 4 workgroups 256 rows apart (k_gb_linear requests the next
                                 round's first chunk under the last products of the current one)
    k_gb_wgrad / k_gen_wgrad     chunks of 32 rows; k_gb_wgrad skips the second 16-row half of a chunk of <= 16 rows
    k_gen_loss                   blocks of 256 rows, the log_std gradient summed per block through an LDS tile [256][A | 1]
PROMP_MAX_CUS=1 plans the tables for one compute unit: every task is one work item, item rows = task rows (pinned on the host by
tests/host/plan_check.cpp; `long_items` below also reads the figure back from a context).  Production shapes on these kernels
(40 tasks x 4000 rows) have ~625 rows per item.

Which shapes run on these kernels is promp_plan.h's pass_family: NOT two plain tanh layers of up to 128 units with obs_dim <= 128 and
act_dim <= 8 -- those are padded onto a fused family.  Every case below says which it is meant to be (`layered`), shape_kwargs
asserts it, and tests/host/plan_check.cpp pins the shapes used here against the C++.

Comparisons and tolerances are parity_checks.check_loss_grad / check_hvp / check_meta / check_dice_path_lengths' own: the float64
oracle (oracle/promp.py, oracle/dice.py), rtol 1e-4 / atol 1e-6 on loss and KL, 1e-4 of the max-norm on gradients and products.
Every check prints its worst figures (profiles/layered_edges.txt keeps a run's).
"""
import functools
import zlib

import numpy as np

from oracle import policy as op
from oracle import promp as pm
from promp_amd import _lib
from tests import helpers, parity_checks as pc

# ---- row-loop edges: path lengths per task; the item row counts sit around 16 / 17 (wgrad's second half), 32 (wgrad chunk), 64 (round),
#      256 (split stride, loss block) and 512
ROW_CASES = {
    # 16, 17, 33, 65 rows: wgrad's second half skipped / not, a second chunk of one row, split 1 with one row
    'A': dict(lengths=[[16], [17], [32, 1], [64, 1]], max_cus=1),
    # 255, 256, 257 rows: all four splits busy, an exact loss block, split 0's second round and a second loss block of one row
    'B': dict(lengths=[[200, 55], [256], [256, 1]], max_cus=1),
    # 321, 513, 1 rows: split 1's second round of one row, a third round, a third loss block, a one-row task beside long ones
    'C': dict(lengths=[[300, 21], [256, 256, 1], [1]], max_cus=1),
    # one task of 513 rows on two compute units: items [0, 256) and [256, 513), their partial rows summed
    'D': dict(lengths=[[513]], max_cus=2),
}
# Column blocks NBW 2 and 1, a scalar-load first layer (9 % 4 != 0), A below 16.  Two plain tanh layers of at most 128 units with
# obs_dim <= 128 and act_dim <= 8 do NOT run layer by layer: pad_dims puts (72, 40) with three actions on the cooperative (128, 128)
# kernels (k_wb_*; tests/host/plan_check.cpp pins both rows).  The same widths with NINE actions stay on k_gb_* / k_gen_* and are
# what reaches the row loops above; the three-action shape is kept beside it (the same item lengths on the cooperative kernels,
# whose rounds are 64 and 32 rows).  `layered` is asserted against helpers.runs_layer_by_layer before a case runs.
ROW_SHAPES = {
    'h72x40_o9_a9': dict(hidden=(72, 40), O=9, A=9, layered=True),
    'h72x40_o9_a3': dict(hidden=(72, 40), O=9, A=3, layered=False),
}
# seeds under which the inputs meet last_row_sensitivity's condition (others put the PPO clip on the longest task's last row: no
# gradient from it under 'clip')
ROW_SEEDS = {('A', 'h72x40_o9_a9'): 702, ('B', 'h72x40_o9_a9'): 715, ('C', 'h72x40_o9_a9'): 702, ('D', 'h72x40_o9_a9'): 704,
             ('A', 'h72x40_o9_a3'): 701, ('B', 'h72x40_o9_a3'): 703, ('C', 'h72x40_o9_a3'): 703, ('D', 'h72x40_o9_a3'): 703}
SHORT = [[65], [16, 17]]                         # width cases: one round + one row; 33 rows in two paths

# ---- width edges: (hidden, O, A, lengths, nonlinearities, with check_meta)
WIDTH_CASES = {
    # scalar loads over two chunks with a one-entry tail (33 = 32 + 1: `k0 + 16 < Kc` false in the second chunk); N = 65: one column in
    # the third 32-column block; K = 65: a weight-gradient slab of one input unit
    # (nine actions keep it layer by layer; with five it is padded onto the cooperative (128, 128) kernels: kept, as ROW_SHAPES')
    'h33x65_o33_a9': dict(hidden=(33, 65), O=33, A=9, lengths=ROW_CASES['B']['lengths'], meta=True),
    'h33x65_o33_a5': dict(hidden=(33, 65), O=33, A=5, lengths=ROW_CASES['B']['lengths'], meta=True, layered=False),
    'h1_o1_a1': dict(hidden=(1,), O=1, A=1, lengths=SHORT),                                   # every width 1
    'h31x32x33_o7_a2': dict(hidden=(31, 32, 33), O=7, A=2, lengths=SHORT),                    # both sides of the 32-column block / 32-entry chunk
    'h129x255_o20_a6': dict(hidden=(129, 255), O=20, A=6, lengths=SHORT),                     # NBW 3 and 4 at odd widths, scalar loads over 5 and 8 chunks
    'h256x4_o20_a6': dict(hidden=(256, 256, 256, 256), O=20, A=6, lengths=SHORT, meta=True),  # the deepest and widest plane layout
    'h64_o1024_a2': dict(hidden=(64,), O=1024, A=2, lengths=SHORT),                           # the obs_dim limit: 16-byte loads, 32 chunks
    'h64_o1023_a2': dict(hidden=(64,), O=1023, A=2, lengths=SHORT),                           # scalar loads, 32 chunks, clamped tail
    # GEN_MAX_A: all 64 column lanes of k_gen_loss, its tile [256][65], an output layer of N = 64; case B's lengths: the per-action
    # column sums run over two blocks
    'h40x40_o12_a64': dict(hidden=(40, 40), O=12, A=64, lengths=ROW_CASES['B']['lengths'], meta=True),
    'h40x40_o12_a63': dict(hidden=(40, 40), O=12, A=63, lengths=SHORT),                       # A odd: the tile's row stride A | 1 is A itself
    'h40x40_o12_a33': dict(hidden=(40, 40), O=12, A=33, lengths=SHORT),
    # the relu / tanh-output epilogues on items of several rounds
    'h64x64_o20_a6_relu_tanh': dict(hidden=(64, 64), O=20, A=6, lengths=ROW_CASES['B']['lengths'], hidden_act='relu', output_act='tanh'),
}


def long_items(monkeypatch, lib, max_cus=1, gen_fp32=False, wide_fp32=None):
    """Plan every context from here on for `max_cus` compute units (PROMP_MAX_CUS), optionally on the exact-FP32 GEMMs
    (PROMP_GEN_FP32=1: k_gen_linear / k_gen_wgrad), and see that a context took the figure: with it ignored the tests of this
    module would run 16-row items and check nothing new.  wide_fp32 (tests/fused_checks.py): True sets PROMP_WIDE_FP32=1 (the
    (128,128) shapes on k_wide_* instead of k_wb_*), False clears it, None leaves it as it is."""
    monkeypatch.setenv('PROMP_MAX_CUS', str(max_cus))
    if gen_fp32:
        monkeypatch.setenv('PROMP_GEN_FP32', '1')
    else:
        monkeypatch.delenv('PROMP_GEN_FP32', raising=False)
    if wide_fp32:
        monkeypatch.setenv('PROMP_WIDE_FP32', '1')
    elif wide_fp32 is not None:
        monkeypatch.delenv('PROMP_WIDE_FP32', raising=False)
    ctx = _lib.Context(1, 3, 2, (8, 8, 8), 1, max_rows=16, max_paths=1, lib=lib)
    try:
        n_cus = ctx.device_info()['n_cus']
    finally:
        ctx.close()
    assert n_cus == max_cus, 'PROMP_MAX_CUS=%d: the context plans for %d compute units' % (max_cus, n_cus)


def shape_kwargs(lengths, hidden, O, A, hidden_act='tanh', output_act=None, layered=True, **_):
    """the arguments of parity_checks' comparisons for one shape on explicit path lengths; `layered`: whether the shape is meant to
    run on the layer-by-layer kernels -- a dispatch that has moved it fails here instead of quietly testing another family"""
    plain = hidden_act == 'tanh' and output_act is None
    assert helpers.runs_layer_by_layer(O, A, hidden, plain) == layered, (hidden, O, A, hidden_act, output_act, layered)
    return dict(M=len(lengths), P=None, T=None, O=O, A=A, hidden=tuple(hidden), lengths_per_task=lengths, hidden_act=hidden_act,
                output_act=output_act)


def report(label, worst, family='layered'):
    print('%s %s: %s' % (family, label, '  '.join('%s %.2e' % kv for kv in sorted(worst.items())) or 'nothing compared'))


def run_check(lib, label, what, seed, shape, family='layered', **kw):
    """one of parity_checks' comparisons on explicit path lengths; its worst figures are printed whether it passes or not
    (loss / kl: fraction of rtol 1e-4 + atol 1e-6; grad / hvp / meta_grad / adapt: of the reference's max-norm, bound 1e-4).
    family: the first word of the printed line (tests/fused_checks.py prints 'fused').  meta: K = 1 and one epoch unless given."""
    worst = {}
    fn = dict(loss_grad=pc.check_loss_grad, hvp=pc.check_hvp, meta=pc.check_meta)[what]
    if what == 'meta':
        kw = dict(dict(K=1, epochs=1), **kw)
    try:
        fn(lib, seed, worst=worst, **dict(shape, **kw))
    finally:
        report('%s %s' % (label, what), worst, family)
    return worst


# ---- a condition on the INPUTS (oracle alone, no kernel): a dropped row must show
def last_row_sensitivity(case, shape):
    """dropped_row_sensitivity for row case `case` at ROW_SHAPES[shape], under the seed ROW_SEEDS holds for the pair"""
    O, A, hidden = (ROW_SHAPES[shape][k] for k in ('O', 'A', 'hidden'))
    return dropped_row_sensitivity(tuple(map(tuple, ROW_CASES[case]['lengths'])), ROW_SEEDS[case, shape], O, A, tuple(hidden))


@functools.lru_cache(maxsize=None)
def dropped_row_sensitivity(lengths, seed, O, A, hidden):
    """By how much (of the gradient's max-norm) the float64 oracle's gradient of the longest task moves when that task loses its last
    row, at check_loss_grad's own inputs (seed, perturbed parameters, step 1's slab) for the path lengths `lengths` (a tuple of
    tuples) at a policy shape: the smallest figure over the three objectives and over two readings of "loses" (the task without the
    row; the row's terms missing from the sums while the mean still divides by the full count, which is what a kernel that skipped
    the row would return -- exactly nothing under 'clip' when the clip is active on that row, so such a seed is not used).
    tests/fused_checks.py asks the same of its own cases."""
    lengths = [list(lens) for lens in lengths]
    theta, all_slabs, _ = helpers.make_promp_case(seed, len(lengths), None, None, O, A, hidden, 1, lengths_per_task=lengths)
    spec = op.PolicySpec(O, A, hidden)
    rng = np.random.RandomState(seed + 1)
    th = (theta + 0.02 * rng.randn(len(lengths), theta.size)).astype(np.float32)
    i = int(np.argmax([sum(lens) for lens in lengths]))
    slab = all_slabs[1][i]
    cut = dict(observations=slab['observations'][:-1], actions=slab['actions'][:-1], advantages=slab['advantages'][:-1],
               agent_infos=dict(mean=slab['agent_infos']['mean'][:-1], log_std=slab['agent_infos']['log_std'][:-1]))
    out = []
    for name in ('ratio', 'clip', 'loglik'):
        full = pm.loss_and_grad(spec, th[i].astype(np.float64), slab, name, False, clip_eps=0.3)['grad']
        less = pm.loss_and_grad(spec, th[i].astype(np.float64), cut, name, False, clip_eps=0.3)['grad']
        n = len(slab['advantages'])
        out += [pc.rel_max(less, full), pc.rel_max(less * (n - 1) / n, full)]
    return min(out)


def check_inputs_show_a_dropped_row(case, shape):
    """ten times the comparison's tolerance: if a seed does not give it, ROW_SEEDS takes another seed, never a smaller bound"""
    moved = last_row_sensitivity(case, shape)
    print('layered rows %s %s: the oracle gradient of the longest task moves by %.2e of its max-norm without its last row' % (case, shape, moved))
    assert moved > 1e-3, (case, shape, moved)


def check_rows(lib, case, shape, what, compact_log_std=False, tag=''):
    """row case A-D at ROW_SHAPES[shape] (the caller has set the switches: long_items(..., ROW_CASES[case]['max_cus']))"""
    check_inputs_show_a_dropped_row(case, shape)
    kw = dict(compact_log_std=True) if compact_log_std else {}
    return run_check(lib, 'rows %s %s%s' % (case, shape, tag), what, ROW_SEEDS[case, shape],
                     shape_kwargs(ROW_CASES[case]['lengths'], **ROW_SHAPES[shape]), **kw)


def check_width(lib, name, what):
    return run_check(lib, 'width %s' % name, what, 800 + zlib.crc32(name.encode()) % 100, shape_kwargs(**WIDTH_CASES[name]))


DICE_LENGTHS = [[256, 65], [64, 1, 129]]      # 321 and 194 rows: row_tan written by k_gen_loss<true, true> over two 256-row blocks


def check_dice(lib):
    """DICE-MAML on the layer-by-layer kernels with long items: a third hidden layer keeps (72, 40, .) off the fused kernels; the
    row tangents k_gen_loss<true, true> writes block by block are read back by k_dice_scan"""
    worst = {}
    try:
        pc.check_dice_path_lengths(lib, 711, DICE_LENGTHS, O=9, A=3, hidden=(72, 40, 24), worst=worst)
    finally:
        report('dice h72x40x24 %s' % DICE_LENGTHS, worst)
    return worst
