"""DiCE sample processing on the device (promp_process_samples_dice / promp_download_dice / promp_use_dice_advantages), shared
by test_emu_dice_processing.py (emulator, the small cases) and test_gpu_dice_processing.py (MI355X, all of them).

References: the reference's own outputs (tests/golden/dice_proc_*.npz) and the float64 restatement oracle.dice.process_samples_dice.
Tolerances are the ones the existing tests apply to the same quantities: adjusted rewards rtol 1e-5 / atol 1e-6 and advantages
rtol 1e-4 / atol 1e-5 (tests/test_plugin_api.py, run_dice_processor_scenario), coefficients rtol 1e-5 / atol 1e-7
(parity_checks.check_sample_processing_golden), installed weights 1e-5 of their largest, an inner step 1e-4 of its max-norm
(run_dice_maml_scenario).
"""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest

from oracle import dice, policy as op, promp as pm, sample_processing as sp
from promp_amd import _lib, synthetic
from tests import helpers
from tests.parity_checks import KIND

ADJ = dict(rtol=1e-5, atol=1e-6)
ADV = dict(rtol=1e-4, atol=1e-5)
COEF = dict(rtol=1e-5, atol=1e-7)
GOLDEN_CASES = ('default', 'ragged', 'raw', 'positive', 'retbase', 'retbase_raw')
EDGE_LENGTHS = [[1, 63, 64, 65, 130], [64, 64]]       # the chunk boundaries of the 64-step scans


def make_ctx(lib, paths, K=1, hidden=(32, 32)):
    fl = _lib.flatten_paths(paths)
    ctx = _lib.Context(len(paths), fl['obs'].shape[1], fl['act'].shape[1], hidden, K, max_rows=len(fl['rew']),
                       max_paths=len(fl['path_row_offsets']) - 1, lib=lib)
    return ctx, fl


def upload(ctx, step, fl):
    ctx.upload_step(step, fl['task_path_offsets'], fl['path_row_offsets'], fl['obs'], fl['rew'], fl['act'], fl['old_mean'], fl['old_log_std'])


def run_dice(lib, paths, T, baseline, return_baseline=None, **kw):
    """one promp_process_samples_dice + promp_download_dice through the C-level calls -> (download, flat arrays)"""
    ctx, fl = make_ctx(lib, paths)
    try:
        upload(ctx, 0, fl)
        ctx.process_samples_dice(0, T, baseline_kind=KIND[baseline],
                                 return_baseline_kind=None if return_baseline is None else KIND[return_baseline], **kw)
        return ctx.download_dice(0), fl
    finally:
        ctx.close()


def assert_padded(rows, pad_value, expected, mask, tol):
    """rows at the valid positions and the pad value at the padded ones equal the padded array `expected`"""
    m = np.asarray(mask) > 0.5
    np.testing.assert_allclose(rows, np.asarray(expected)[m], **tol)
    if not m.all():
        np.testing.assert_allclose(np.full(int((~m).sum()), pad_value), np.asarray(expected)[~m], **tol)


def oracle_coeffs(plist, T, discount, kind, returns=False, reg=1e-5):
    obs = [np.asarray(p['observations']) for p in plist]
    if returns:
        tgt = [sp.discount_cumsum(np.asarray(p['rewards'], dtype=np.float64), discount) for p in plist]
    else:
        disc = np.cumprod(np.concatenate([np.ones(1), np.ones(T - 1) * discount]))
        tgt = [np.asarray(p['rewards'], dtype=np.float64) * disc[:len(p['rewards'])] for p in plist]
    return sp.fit_linear_baseline(obs, tgt, KIND[kind], reg)[0]


def compare(out, fl, paths, expected, T, baseline, return_baseline, discount):
    """expected: per task dict(mask, adjusted_rewards[, advantages])"""
    pro, tpo = fl['path_row_offsets'], fl['task_path_offsets']
    for i, plist in enumerate(paths.values()):
        r0, r1 = pro[tpo[i]], pro[tpo[i + 1]]
        e = expected[i]
        assert_padded(out['adjusted'][r0:r1], out['pad_adjusted'][i], e['adjusted_rewards'], e['mask'], ADJ)
        if return_baseline is not None:
            assert_padded(out['advantages'][r0:r1], out['pad_advantages'][i], e['advantages'], e['mask'], ADV)
            if return_baseline != 'zero':
                np.testing.assert_allclose(out['return_coeffs'][i], oracle_coeffs(plist, T, discount, return_baseline, returns=True), **COEF)
        if baseline != 'zero':
            np.testing.assert_allclose(out['coeffs'][i], oracle_coeffs(plist, T, discount, baseline), **COEF)
    und = [np.sum(np.asarray(p['rewards'], dtype=np.float64)) for plist in paths.values() for p in plist]
    np.testing.assert_allclose(out['path_undiscounted'], und, rtol=1e-12, atol=1e-12)


# ---- 1. the reference's own outputs --------------------------------------------------------------------------------------
def check_golden(lib, name):
    g = np.load(os.path.join(helpers.GOLDEN, 'dice_proc_%s.npz' % name))
    meta = json.loads(str(g['meta']))
    paths = helpers.dice_paths_from_golden(g)
    T, kw = meta['max_path_length'], dict(meta['kwargs'])
    out, fl = run_dice(lib, paths, T, meta['baseline'], meta.get('return_baseline'), **kw)
    expected = [dict(mask=g['mask'][i], adjusted_rewards=g['adjusted_rewards'][i],
                     **(dict(advantages=g['advantages'][i]) if meta.get('return_baseline') else {})) for i in range(len(paths))]
    compare(out, fl, paths, expected, T, meta['baseline'], meta.get('return_baseline'), kw.get('discount', 0.99))


# ---- 2. scan and padding edges -------------------------------------------------------------------------------------------
def edge_paths(seed, lengths_per_task, O=4, A=2, hidden=(32, 32), rewards='normal'):
    rng = np.random.RandomState(seed)
    theta = synthetic.init_theta(rng, O, hidden, A)
    paths = helpers.make_paths_with_lengths(rng, theta, lengths_per_task, O, A, hidden)
    for plist in paths.values():
        for p in plist:
            r = rng.randn(len(p['rewards']))
            p['rewards'] = (np.abs(r) + 0.1 if rewards == 'positive' else r).astype(np.float32)
    return paths, theta


def oracle_dice(paths, T, baseline, return_baseline=None, discount=0.97, gae_lambda=0.9, normalize_adv=True, positive_adv=False):
    return [dice.process_samples_dice(plist, T, baseline_kind=KIND[baseline], discount=discount, normalize_adv=normalize_adv,
                                      positive_adv=positive_adv,
                                      return_baseline_kind=None if return_baseline is None else KIND[return_baseline],
                                      gae_lambda=gae_lambda) for plist in paths.values()]


def min_is_padding(sd, raw):
    """which branch of the minimum the padded array of adjusted rewards takes: True = a padded zero, False = a valid entry"""
    m = np.asarray(sd['mask']) > 0.5
    a = np.asarray(raw['adjusted_rewards'])
    return (not m.all()) and a[~m].min() <= a[m].min()


def check_edges(lib, T, baseline, rewards, normalize_adv, positive_adv, return_baseline='linear_feature', expect_min_padding=None,
                lengths=EDGE_LENGTHS):
    kw = dict(discount=0.97, gae_lambda=0.9, normalize_adv=normalize_adv, positive_adv=positive_adv)
    paths, _ = edge_paths(7, lengths, rewards=rewards)
    expected = oracle_dice(paths, T, baseline, return_baseline, **kw)
    if expect_min_padding is not None:          # the input still covers the branch it is here for (task 0 holds the edge lengths)
        raw = oracle_dice(paths, T, baseline, None, **dict(kw, normalize_adv=False, positive_adv=False))
        assert min_is_padding(expected[0], raw[0]) == expect_min_padding
    out, fl = run_dice(lib, paths, T, baseline, return_baseline, **kw)
    compare(out, fl, paths, expected, T, baseline, return_baseline, 0.97)


def check_unpadded_task(lib):
    """[64, 64] at max_path_length 64: no padding anywhere, the minimum must ignore zero (all adjusted rewards positive)"""
    kw = dict(discount=0.97, gae_lambda=0.9, normalize_adv=False, positive_adv=True)
    paths, _ = edge_paths(8, [[64, 64]], rewards='positive')
    expected = oracle_dice(paths, 64, 'zero', 'zero', **kw)
    assert np.asarray(expected[0]['mask']).all()
    out, fl = run_dice(lib, paths, 64, 'zero', 'zero', **kw)
    compare(out, fl, paths, expected, 64, 'zero', 'zero', 0.97)
    assert out['adjusted'].min() == pytest.approx(1e-8, rel=1e-6)      # shifted by the valid minimum, not by zero


# ---- 3. installed weights -------------------------------------------------------------------------------------------------
def check_installed_weights(lib, T=160):
    kw = dict(discount=0.97, gae_lambda=0.9, normalize_adv=True, positive_adv=False)
    O, A, hidden = 4, 2, (32, 32)
    paths, theta = edge_paths(9, EDGE_LENGTHS, O, A, hidden)
    slabs = [dice.to_slab(sd) for sd in oracle_dice(paths, T, 'linear_feature', 'linear_feature', **kw)]
    w = np.concatenate([sl['advantages'] for sl in slabs])
    vpg = np.concatenate([sl['vpg_advantages'] for sl in slabs])
    rw = np.concatenate([sl['dice_rw'] for sl in slabs])
    ctx, fl = make_ctx(lib, paths, hidden=hidden)
    try:
        ctx.set_theta(theta)
        ctx.set_step_sizes(np.full(ctx.n_params, 0.1, np.float32))

        def inner_step():
            ctx.switch_to_pre_update()
            ctx.inner_adapt(0, _lib.INNER_DICE)
            return ctx.get_task_thetas().astype(np.float64) - theta.astype(np.float64)
        upload(ctx, 0, fl)
        ctx.set_dice_rewards(0, rw.astype(np.float32))                    # the old route
        old = inner_step()
        upload(ctx, 0, fl)
        ctx.process_samples_dice(0, T, baseline_kind=KIND['linear_feature'], return_baseline_kind=KIND['linear_feature'], **kw)
        got = ctx.download_processed(0, KIND['linear_feature'])['advantages']
        assert np.max(np.abs(got - w)) <= 1e-5 * np.max(np.abs(w))
        new = inner_step()
        assert np.max(np.abs(new - old)) <= 1e-4 * np.max(np.abs(old))
        ctx.use_dice_advantages(0)
        got = ctx.download_processed(0, KIND['linear_feature'])['advantages']
        assert np.max(np.abs(got - vpg)) <= 1e-5 * np.max(np.abs(vpg))
    finally:
        ctx.close()


# ---- 4. reserved == 0 is the old call -------------------------------------------------------------------------------------
def check_plain_call_unchanged(lib):
    meta, paths, _ = helpers.load_sample_proc('ragged')
    for plist in paths.values():
        for p in plist:
            p['actions'] = p['actions'].astype(np.float32)
    ctx, fl = make_ctx(lib, paths)
    try:
        def plain():
            upload(ctx, 0, fl)
            ctx.process_samples(0, baseline_kind=KIND[meta['baseline']], **meta['kwargs'])
            out = ctx.download_processed(0)
            ret64, adv64 = ctx.download_raw(0)
            return [np.array(x) for x in (out['returns'], out['advantages'], out['coeffs'], ret64, adv64)]
        before = plain()
        upload(ctx, 1, fl)
        longest = int(np.diff(fl['path_row_offsets']).max())
        ctx.process_samples_dice(1, longest + 3, baseline_kind=KIND['linear_feature'], return_baseline_kind=KIND['linear_time'])
        ctx.download_dice(1)
        after = plain()
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
    finally:
        ctx.close()


# ---- 5. residency through the plugin --------------------------------------------------------------------------------------
def _plugin(M, O, A, hidden, T, vpg):
    from promp_amd.baselines.linear_baseline import LinearFeatureBaseline
    from promp_amd.meta_algos.dice_maml import DICEMAML
    from promp_amd.meta_algos.vpg_dice_maml import VPG_DICEMAML
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.dice_sample_processor import DiceMetaSampleProcessor
    from promp_amd.utils import logger
    logger.configure(quiet=True)
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=O, action_dim=A, meta_batch_size=M, hidden_sizes=hidden)
    extra = dict(return_baseline=LinearFeatureBaseline()) if vpg else {}
    proc = DiceMetaSampleProcessor(LinearFeatureBaseline(), max_path_length=T, discount=0.97, gae_lambda=0.9, normalize_adv=True, **extra)
    algo = (VPG_DICEMAML if vpg else DICEMAML)(T, policy=policy, learning_rate=1e-3, inner_lr=0.1, meta_batch_size=M, num_inner_grad_steps=1)
    return policy, proc, algo


def check_plugin_residency(make_batches, M, O, A, hidden, T, vpg):
    """make_batches(policy) -> [batch of step 0, batch of step 1], each a DevicePaths resident in its slot.  The processor and the
    algorithm upload nothing; the samples equal the upload route's; VPG's loss equals the oracle's on them."""
    policy, proc, algo = _plugin(M, O, A, hidden, T, vpg)
    sess = policy.session
    spec = op.PolicySpec(O, A, hidden)
    theta = spec.from_ordered_dict(policy.get_param_values()).astype(np.float64)
    policy.switch_to_pre_update()
    batches = make_batches(policy)
    count = sess._upload_counter
    samples = []
    for k, batch in enumerate(batches):
        sds = proc.process_samples(batch, log=False)
        assert sess._upload_counter == count
        assert all(sd.device_ref[:3] == tuple(batch.device_ref) for sd in sds) and [sd.device_ref[3] for sd in sds] == list(range(M))
        samples.append(sds)
        if k == 0:
            algo._adapt(sds)
    algo.optimize_policy(samples, log=False)
    assert sess._upload_counter == count
    if vpg:
        slabs = [[dice.to_slab(sd) for sd in step] for step in samples]
        r = dice.meta_objective_and_grad(spec, theta, slabs, np.full(spec.n_params, 0.1), want_grad=False, outer='vpg')
        np.testing.assert_allclose(algo.last_stats['loss_before'], r['loss'], rtol=1e-4, atol=1e-6)
    # the same paths as a plain dict take the upload route and give the same arrays
    for batch, sds in zip(batches, samples):
        plain = OrderedDict((i, [dict(p) for p in plist]) for i, plist in batch.items())
        ups = proc.process_samples(plain, log=False)
        assert sess._upload_counter == count + 1
        count += 1
        for a, b in zip(sds, ups):
            np.testing.assert_array_equal(a['mask'], b['mask'])
            np.testing.assert_array_equal(a['observations'], b['observations'])
            np.testing.assert_allclose(a['adjusted_rewards'], b['adjusted_rewards'], **ADJ)
            if vpg:
                np.testing.assert_allclose(a['advantages'], b['advantages'], **ADV)
    import promp_amd.session as session_mod
    if sess.ctx is not None:
        sess.ctx.close()
    session_mod._current = None


def hand_built_batches(M, O, A, hidden, lengths):
    """emulator: DevicePaths around a session.upload_flat, so that no rollout kernel has to run"""
    from promp_amd.samplers.device_point_sampler import DevicePaths

    def make(policy):
        sess, out = policy.session, []
        rng = np.random.RandomState(11)
        theta = synthetic.init_theta(rng, O, hidden, A)
        for slot in range(2):
            paths = helpers.make_paths_with_lengths(rng, theta, lengths, O, A, hidden)
            fl = _lib.flatten_paths(paths)
            sess.upload_flat(slot, fl)
            dp = DevicePaths(paths)
            dp.device_ref, dp.flat = (sess.serial, sess.upload_serial[slot], slot), fl
            out.append(dp)
        return out
    return make


def point_env_batches(M, B, T):
    """GPU: two sampling steps of DevicePointEnvSampler"""
    from promp_amd.envs.point_env import MetaPointEnvCorner
    from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler

    def make(policy):
        np.random.seed(5)
        sampler = DevicePointEnvSampler(env=MetaPointEnvCorner(reward_type='dense'), policy=policy, rollouts_per_meta_task=B,
                                        meta_batch_size=M, max_path_length=T)
        sampler.update_tasks()
        return [sampler.obtain_samples(), sampler.obtain_samples()]
    return make


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def check_refusals(lib):
    paths, _ = edge_paths(12, [[5, 9], [7]])
    ctx, fl = make_ctx(lib, paths)
    try:
        upload(ctx, 0, fl)
        with pytest.raises(_lib.PrompError, match='max_path_length'):
            ctx.process_samples_dice(0, 8)
        with pytest.raises(_lib.PrompError, match='baseline kind 7'):
            ctx.process_samples_dice(0, 9, baseline_kind=7)
        with pytest.raises(_lib.PrompError, match='return baseline kind 5'):
            ctx.process_samples_dice(0, 9, return_baseline_kind=5)
        with pytest.raises(_lib.PrompError, match='no data'):
            ctx.process_samples_dice(1, 9)                 # never uploaded
        ctx.process_samples_dice(0, 9, baseline_kind=KIND['linear_time'])
        with pytest.raises(_lib.PrompError, match='return baseline'):
            ctx.use_dice_advantages(0)
        out = ctx.download_dice(0)                    # the context is still usable
        assert np.all(np.isfinite(out['adjusted'])) and out['advantages'] is None
    finally:
        ctx.close()


# ---- 7. one case per Gram / fit family (GPU) ------------------------------------------------------------------------------
def check_family(lib, O):
    kw = dict(discount=0.97, gae_lambda=0.9, normalize_adv=True, positive_adv=False)
    paths, _ = edge_paths(13 + O, [[30, 64, 65, 100]], O=O, A=2)
    expected = oracle_dice(paths, 100, 'linear_feature', None, **kw)
    out, fl = run_dice(lib, paths, 100, 'linear_feature', None, **kw)
    compare(out, fl, paths, expected, 100, 'linear_feature', None, 0.97)
