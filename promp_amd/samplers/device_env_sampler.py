"""Rollouts of an environment that LIVES ON THE GPU, collected without a host hop per step.

DeviceSlabSampler serves environments the host steps: every vectorised step uploads the observations, downloads the actions and
synchronises.  A simulator that already runs on the same GPU -- a vectorised environment written with torch tensors on ROCm, a
kernel of the user's -- hands device arrays over instead:

    ctx.policy_step_dev(slot, s, obs, actions, ...)       # mean network, exploration noise, staging rows: one launch, no copy
    obs, rewards, done = vec_env.step(actions)            # the simulator's own launches, on its own stream
    ctx.file_step_dev(slot, s, rewards, done, T, ended)   # reward and episode end filed under (s, environment): one launch
    obs = vec_env.reset_where(ended)

Nothing in this loop waits for the GPU: the library orders its stream against the simulator's with two events per call
(promp_hip.h, (c)).  The stop rule of the reference's sampler (meta_sampler.py:100-125: stop once total_samples steps lie in
FINISHED episodes, drop what is still running) is evaluated on the device over the filed steps; the host asks for it
(collection_progress, the loop's only synchronisation) first at step ceil(total_samples / n_envs) - 1, the earliest step that can
be the stop step, then every `poll_every` steps, and gives up at max_steps = T - 1 + ceil(total_samples / n_envs), which always
suffices.  Steps filed beyond the stop step are ignored.  end_collection_dev then builds the path tables and copies the finished
episodes into the sampling step's slab on the device, where MetaSampleProcessor.process_samples and _adapt find them resident.

The vec_env protocol (duck-typed):

    vec_env.n_envs                   meta_batch_size * envs_per_task; environment e = task * envs_per_task + b
    vec_env.set_tasks(tasks)         one task per meta-batch slot, as env.sample_tasks(meta_batch_size) returned them
    vec_env.reset() -> obs           every environment starts an episode; obs [n_envs, obs_dim] float32
    vec_env.step(actions) -> (obs, rewards, done)
                                     actions [n_envs, act_dim] float32; obs the observation AFTER the step, rewards [n_envs] float32,
                                     done [n_envs] uint8 (or None: episodes end by max_path_length alone)
    vec_env.reset_where(ended) -> obs
                                     ended [n_envs] uint8: the environments whose episode ended with the last step (done, or
                                     max_path_length reached) start their next one; obs is what the policy sees next
    vec_env.stream                   optional: the stream the simulator enqueues on (an int handle or an object with .cuda_stream);
                                     absent / None: the null stream
    vec_env.empty(shape, dtype)      optional: allocates `actions` and `ended` as the simulator's own array type; absent: they are
                                     promp_amd._lib.DeviceArray, which carry __cuda_array_interface__

Every array is a float32 or uint8 DEVICE array: a DeviceArray, a torch tensor on the GPU, or anything with
__cuda_array_interface__ (_lib.device_pointer refuses everything else by name -- a NumPy array never reaches a kernel).  The
arrays returned by one call must stay valid until the next call of the same method (the library reads them in stream order).

Not served here: the normalize wrapper's running moments for an external environment, env_infos (empty dicts), float64 rewards,
an environment sharded over several ranks.
"""
import numpy as np

from ..utils import logger
from .device_point_sampler import DevicePaths


class DeviceEnvSampler(object):
    def __init__(self, vec_env, env, policy, rollouts_per_meta_task, meta_batch_size, max_path_length, envs_per_task=None,
                 poll_every=8):
        missing = [name for name in ('n_envs', 'set_tasks', 'reset', 'step', 'reset_where') if not hasattr(vec_env, name)]
        assert not missing, 'vec_env lacks %s' % ', '.join(missing)
        assert hasattr(env, 'sample_tasks'), 'env draws the tasks: it needs sample_tasks(n)'
        self.vec_env, self.env, self.policy = vec_env, env, policy
        self.batch_size = rollouts_per_meta_task
        self.meta_batch_size = meta_batch_size
        self.max_path_length = max_path_length
        self.envs_per_task = rollouts_per_meta_task if envs_per_task is None else int(envs_per_task)
        assert int(vec_env.n_envs) == meta_batch_size * self.envs_per_task, \
            'vec_env has %d environments, meta_batch_size * envs_per_task = %d' % (vec_env.n_envs, meta_batch_size * self.envs_per_task)
        assert int(poll_every) >= 1
        self.poll_every = int(poll_every)
        self.total_samples = meta_batch_size * rollouts_per_meta_task * max_path_length
        self.total_timesteps_sampled = 0
        self.last_seed = None
        self.last_n_steps = None           # vectorised steps the last collection kept (stop step + 1) / filed
        self.last_steps_filed = None
        self._bufs = None                  # (context, actions, ended)

    def update_tasks(self):
        tasks = self.env.sample_tasks(self.meta_batch_size)
        assert len(tasks) == self.meta_batch_size
        self.vec_env.set_tasks(tasks)

    def _buffers(self, ctx):
        if self._bufs is None or self._bufs[0] is not ctx:
            n, A = self.meta_batch_size * self.envs_per_task, self.policy.action_dim
            empty = getattr(self.vec_env, 'empty', None) or ctx.device_array
            self._bufs = (ctx, empty((n, A), np.float32), empty((n,), np.uint8))
        return self._bufs[1], self._bufs[2]

    def obtain_samples(self, log=False, log_prefix=''):
        M, B, T = self.meta_batch_size, self.envs_per_task, self.max_path_length
        n_envs, total = M * B, self.total_samples
        first_poll = -(-total // n_envs) - 1       # no earlier step can be the stop step: s + 1 steps hold at most n_envs (s + 1) rows
        max_steps = T - 1 + -(-total // n_envs)    # (the bound of DeviceSlabSampler)
        sess = self.policy.session
        ctx = sess.ensure(max_steps * n_envs, max_steps * n_envs)
        if sess.task_thetas is not None:           # parameters set while no context existed yet
            ctx.set_task_thetas(sess.task_thetas)
            sess.task_thetas = None
        slot = sess.next_slot()
        ctx.begin_collection(slot, B, max_steps)
        self.last_seed = seed = int(np.random.randint(0, 2 ** 31 - 1))
        stream = getattr(self.vec_env, 'stream', None)
        actions, ended = self._buffers(ctx)
        clip_infos = self.policy._pre_update_mode
        obs = self.vec_env.reset()
        s, next_poll = 0, first_poll
        while True:
            ctx.policy_step_dev(slot, s, obs, actions, seed=seed, clip_infos=clip_infos, stream=stream)
            obs, rewards, done = self.vec_env.step(actions)
            ctx.file_step_dev(slot, s, rewards, done, T, ended, stream=stream)
            if s + 1 == max_steps:
                break
            if s == next_poll:                     # the loop's only synchronisation
                if ctx.collection_progress(slot, total)[0] >= 0:
                    break
                next_poll += self.poll_every
            obs = self.vec_env.reset_where(ended)
            s += 1
        try:
            tables = ctx.end_collection_dev(slot, total)
        except RuntimeError as e:
            if 'no finished episode' not in str(e):
                raise
            raise RuntimeError('DeviceEnvSampler: %s (rollouts_per_meta_task = %d, max_path_length = %d)' % (e, self.batch_size, T))
        self.last_n_steps, self.last_steps_filed = tables['n_steps'], s + 1
        sess._upload_counter += 1
        sess.upload_serial[slot] = sess._upload_counter
        slab = ctx.download_step(slot)
        tpo, pro = tables['task_path_offsets'], tables['path_row_offsets']
        paths = DevicePaths()
        for i in range(M):
            paths[i] = []
            for p in range(tpo[i], tpo[i + 1]):
                rows = slice(pro[p], pro[p + 1])
                paths[i].append(dict(observations=slab['obs'][rows], actions=slab['act'][rows], rewards=slab['rew'][rows],
                                     env_infos={},
                                     agent_infos=dict(mean=slab['old_mean'][rows],
                                                      log_std=np.tile(slab['old_log_std'][i], (pro[p + 1] - pro[p], 1)))))
        paths.device_ref = (sess.serial, sess.upload_serial[slot], slot)
        paths.flat = dict(task_path_offsets=tpo, path_row_offsets=pro, path_env=tables['path_env'], path_start=tables['path_start'],
                          obs=slab['obs'], act=slab['act'], rew=slab['rew'], old_mean=slab['old_mean'], old_log_std=slab['old_log_std'])
        self.total_timesteps_sampled += self.total_samples
        if log:
            logger.logkv(log_prefix + 'PolicyExecTime', 0.0)
            logger.logkv(log_prefix + 'EnvExecTime', 0.0)
        return paths
