"""DiceSampleProcessor / DiceMetaSampleProcessor (reference: meta_policy_search/samplers/dice_sample_processor.py:6-230,
samplers/meta_sample_processor.py:50-51).

Contract: discounted rewards r_t gamma^t, a reward baseline fitted on them, adjusted rewards = discounted reward - baseline,
every path zero-padded to max_path_length with a mask, adjusted rewards normalised / shifted over the PADDED [paths,
max_path_length] array, path statistics logged from the discounted rewards.

Where the arithmetic runs: on the device, in one call (promp_process_samples_dice: discounted rewards, baseline fit, adjusted
rewards, the normalisation over the padded array from the paths' moments, the DiCE rewards of the valid rows and their suffix
sums; with a return_baseline also returns, fit, GAE and the padded normalisation of the advantages), on the step's slab -- a
batch a device sampler left resident (DevicePaths) is not uploaded, anything else is uploaded once, with its true rewards.  One
download brings the valid rows and each task's pad value back; masks and the padded copies of the inputs are array bookkeeping
on the host.  DICEMAML._adapt / optimize_policy find the slab and its DiCE rewards resident; VPG_DICEMAML finds the advantages
beside them (promp_use_dice_advantages).  The path dicts' 'adjusted_rewards' are the rows of the samples' array (normalised /
shifted wherever the processor does either).
"""
from collections import OrderedDict

import numpy as np

from .. import _lib, session as session_mod
from .base import SampleProcessor, _concat_tensor_dict_list, _log_return_stats


class DiceSamplesData(session_mod.SamplesData):
    """padded samples of one task (mask, observations, actions, rewards, adjusted_rewards, env_infos, agent_infos)"""


class DiceSampleProcessor(SampleProcessor):
    """Args (dice_sample_processor.py:25-47): baseline, max_path_length, discount=0.99, gae_lambda=1, normalize_adv=True,
    positive_adv=False, return_baseline=None

    return_baseline (dice_sample_processor.py:113-124, 196-238): a second baseline, fitted on the returns, adds GAE
    'advantages' (padded, normalised / shifted over the padded array) beside the DiCE rewards -- what VPG_DICEMAML's outer
    objective reads.  Its regression and the GAE scan are a second run of the device pipeline on the same resident slab."""

    def __init__(self, baseline, max_path_length, discount=0.99, gae_lambda=1, normalize_adv=True, positive_adv=False,
                 return_baseline=None):
        assert 0 <= discount <= 1.0, 'discount factor must be in [0,1]'
        assert max_path_length > 0
        assert hasattr(baseline, 'fit') and hasattr(baseline, 'predict')
        super(DiceSampleProcessor, self).__init__(baseline, discount=discount, gae_lambda=gae_lambda, normalize_adv=normalize_adv,
                                                  positive_adv=positive_adv)
        self.max_path_length = max_path_length
        if return_baseline is not None:
            assert hasattr(return_baseline, 'fit') and hasattr(return_baseline, 'predict')
        self.return_baseline = return_baseline

    def _baseline_kind(self):
        """The regression runs on the device, so the baseline must be one the device knows (the `kind` of LinearFeatureBaseline /
        LinearTimeBaseline / ZeroBaseline).  Anything else would silently act as a zero baseline: refuse it instead."""
        kind = getattr(self.baseline, 'kind', None)
        if kind is None:
            raise TypeError('%s has no device-side `kind`: the DiCE sample processor fits its baseline on the device and takes '
                            'promp_amd.baselines.{LinearFeatureBaseline, LinearTimeBaseline, ZeroBaseline}' % type(self.baseline).__name__)
        return kind

    # -- padded arrays ---------------------------------------------------------------------------------------------------
    def _pad(self, array, path_length):
        array = np.asarray(array)
        assert path_length == array.shape[0]
        if array.ndim not in (1, 2):
            raise NotImplementedError
        return np.pad(array, ((0, self.max_path_length - path_length),) + ((0, 0),) * (array.ndim - 1), mode='constant')

    def _stack_padded(self, plist, key, sub=None):
        get = (lambda p: p[key][sub]) if sub is not None else (lambda p: p[key])
        return np.stack([self._pad(get(p), len(p['rewards'])) for p in plist], axis=0)

    def _process_meta_batch(self, paths_meta_batch):
        """-> (list of DiceSamplesData per task, all paths with 'discounted_rewards' / 'adjusted_rewards' added)"""
        T = self.max_path_length
        M = len(paths_meta_batch)
        if hasattr(paths_meta_batch, 'settle'):
            paths_meta_batch.settle()             # a pending side effect of an earlier processor goes in first: this call adds its own
        path_lists = list(paths_meta_batch.values())
        kind, rkind = self._baseline_kind(), None
        if self.return_baseline is not None:
            rkind = getattr(self.return_baseline, 'kind', None)
            if rkind is None:
                raise TypeError('%s has no device-side `kind`' % type(self.return_baseline).__name__)
        opts = dict(max_path_length=T, discount=self.discount, gae_lambda=self.gae_lambda, normalize_adv=self.normalize_adv,
                    positive_adv=self.positive_adv, baseline_kind=kind, reg_coeff=getattr(self.baseline, '_reg_coeff', 1e-5),
                    return_baseline_kind=rkind, return_reg_coeff=getattr(self.return_baseline, '_reg_coeff', 1e-5))
        # the resident test of SampleProcessor._process_on_device: a batch a device sampler wrote into its slab is not uploaded
        sess, ref = session_mod.current(), getattr(paths_meta_batch, 'device_ref', None)
        resident = ref is not None and sess is not None and sess.ctx is not None and ref[0] == sess.serial \
            and sess.upload_serial[ref[2]] == ref[1]
        if resident:
            fl, upload, slot = paths_meta_batch.flat, ref[1], ref[2]
        else:
            fl = _lib.flatten_paths(paths_meta_batch)
        pro, tpo = np.asarray(fl['path_row_offsets']), np.asarray(fl['task_path_offsets'])
        lens_all = np.diff(pro)
        assert T >= int(lens_all.max()), 'a path is longer than max_path_length'
        if not resident:
            first = path_lists[0][0]
            A = int(np.asarray(first['actions']).reshape(len(first['rewards']), -1).shape[1])
            sess = self._session_for(M, fl['obs'].shape[1], A)
            slot = sess.next_slot()
            upload = sess.upload_flat(slot, fl)        # the true rewards: the device forms the discounted ones itself
        ctx = sess.ctx
        ctx.process_samples_dice(slot, **opts)
        # host work while the device is busy: the discounted rewards of the path dicts, masks, padded copies of the inputs
        disc = np.cumprod(np.concatenate([np.ones(1), np.ones(T - 1) * self.discount]))
        padded = []
        for i, plist in enumerate(path_lists):
            for p in plist:
                p['discounted_rewards'] = np.asarray(p['rewards']) * disc[:len(p['rewards'])]
            lens = lens_all[tpo[i]:tpo[i + 1]]
            padded.append(dict(
                mask=(np.arange(T)[None, :] < lens[:, None]).astype(np.float64),
                observations=self._stack_padded(plist, 'observations'),
                actions=self._stack_padded(plist, 'actions'),
                rewards=self._stack_padded(plist, 'rewards'),
                env_infos={k: self._stack_padded(plist, 'env_infos', k) for k in plist[0].get('env_infos', {})},
                agent_infos={k: self._stack_padded(plist, 'agent_infos', k) for k in plist[0].get('agent_infos', {})}))
        out = ctx.download_dice(slot)
        if kind != _lib.BASELINE_ZERO:
            self.baseline._coeffs = out['coeffs'][-1].copy()       # the shared baseline ends on the last task's fit
        ret64 = gae = None
        if rkind is not None:
            if rkind != _lib.BASELINE_ZERO:
                self.return_baseline._coeffs = out['return_coeffs'][-1].copy()
            ret64, gae = ctx.download_raw(slot)                     # the path dicts' float64 returns and raw GAE advantages

        def pad_rows(rows, mask, pad_value):
            a = np.full(mask.shape, pad_value, dtype=np.float64)
            a[mask > 0.5] = rows                                     # path-major, time-major: the slab's order
            return a
        result = []
        ends = pro.tolist()
        for i, plist in enumerate(path_lists):
            for j, p in enumerate(plist):
                a, b = ends[tpo[i] + j], ends[tpo[i] + j + 1]
                # (the rows of the samples' array: normalised / shifted wherever the processor does either)
                p['adjusted_rewards'] = out['adjusted'][a:b]
                if gae is not None:
                    p['returns'], p['advantages'] = ret64[a:b], gae[a:b]
            r0, r1 = ends[tpo[i]], ends[tpo[i + 1]]
            sd = DiceSamplesData(adjusted_rewards=pad_rows(out['adjusted'][r0:r1], padded[i]['mask'], out['pad_adjusted'][i]), **padded[i])
            if rkind is not None:
                sd['advantages'] = pad_rows(out['advantages'][r0:r1], padded[i]['mask'], out['pad_advantages'][i])
            sd.device_ref = (sess.serial, upload, slot, i)
            sd.dice_advantages_resident = rkind is not None         # VPG_DICEMAML: promp_use_dice_advantages instead of an upload
            result.append(sd)
        return result, [p for plist in path_lists for p in plist]

    # -- reference API ---------------------------------------------------------------------------------------------------
    def process_samples(self, paths, log=False, log_prefix=''):
        """single task: list of paths -> padded samples dict (dice_sample_processor.py:49-90)"""
        assert type(paths) == list, 'paths must be a list'
        assert paths[0].keys() >= {'observations', 'actions', 'rewards'}
        assert self.baseline, 'baseline must be specified - use self.build_sample_processor(baseline_obj)'
        result, all_paths = self._process_meta_batch(OrderedDict([(0, paths)]))
        self._log_dice_stats(all_paths, log=log, log_prefix='')   # the reference drops log_prefix here (:87)
        sd = dict(result[0])
        assert sd.keys() >= {'observations', 'actions', 'rewards', 'adjusted_rewards', 'mask'}
        return sd

    def _log_dice_stats(self, paths, log=False, log_prefix=''):
        """dice_sample_processor.py:133-147 ('discounted return' = the sum of a path's discounted rewards)"""
        _log_return_stats(self._stat_session(), [np.sum(p['rewards']) for p in paths],
                          [np.sum(p['discounted_rewards']) for p in paths], log, log_prefix)


class DiceMetaSampleProcessor(DiceSampleProcessor):
    """MetaSampleProcessor.process_samples on the DiCE processor (samplers/meta_sample_processor.py:8-51)"""

    def process_samples(self, paths_meta_batch, log=False, log_prefix=''):
        assert isinstance(paths_meta_batch, dict), 'paths must be a dict'
        assert self.baseline, 'baseline must be specified'
        samples_data_meta_batch, all_paths = self._process_meta_batch(paths_meta_batch)
        # rewards z-scored over the whole meta-batch (meta_sample_processor.py:40-44), here on the padded reward arrays
        overall = np.concatenate([sd['rewards'].reshape(-1) for sd in samples_data_meta_batch])
        sess = self._stat_session()
        if sess.world == 1:
            mean, std = np.mean(overall), np.std(overall)
        else:           # task-sharded: the padded arrays of the other ranks' tasks enter through their moments
            n, s1, s2 = sess.allreduce([overall.size, np.sum(overall, dtype=np.float64), np.sum(overall.astype(np.float64) ** 2)])
            mean = s1 / n
            std = np.sqrt(max(s2 / n - mean * mean, 0.0))
        for sd in samples_data_meta_batch:
            sd['adj_avg_rewards'] = (sd['rewards'] - mean) / (std + 1e-8)
        self._log_dice_stats(all_paths, log=log, log_prefix=log_prefix)
        return samples_data_meta_batch
