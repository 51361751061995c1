#!/usr/bin/env python
"""ProMP on a point-mass environment that LIVES ON THE GPU as torch tensors (promp_amd/envs/torch_point_env.py: MetaPointEnvV2's
dynamics), collected through DeviceEnvSampler: observations, actions, rewards and `done` flags never leave the device, and the
sampling loop does not wait for it between steps.  An example of plugging a simulator of your own into the library; needs
torch for ROCm (the package itself does not).

    python run_scripts/pro-mp_run_torch_point_mass.py [--config_file cfg.json] [--dump_path DIR] [--n_itr N]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from promp_amd.baselines.linear_baseline import LinearFeatureBaseline  # noqa: E402
from promp_amd.envs.point_env import MetaPointEnvV2  # noqa: E402
from promp_amd.meta_algos.pro_mp import ProMP  # noqa: E402
from promp_amd.meta_trainer import Trainer  # noqa: E402
from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy  # noqa: E402
from promp_amd.samplers.device_env_sampler import DeviceEnvSampler  # noqa: E402
from promp_amd.samplers.meta_sample_processor import MetaSampleProcessor  # noqa: E402
from promp_amd.utils import logger  # noqa: E402

DEFAULT = {
    'seed': 1, 'rollouts_per_meta_task': 20, 'envs_per_task': None, 'max_path_length': 100, 'poll_every': 8,
    'discount': 0.99, 'gae_lambda': 1, 'normalize_adv': True,
    'hidden_sizes': (32, 32),
    'inner_lr': 0.1, 'learning_rate': 1e-3, 'num_promp_steps': 5, 'clip_eps': 0.3, 'target_inner_step': 0.01,
    'init_inner_kl_penalty': 5e-4, 'adaptive_inner_kl_penalty': False,
    'n_itr': 100, 'meta_batch_size': 40, 'num_inner_grad_steps': 1,
    'own_stream': True,            # the environment enqueues on a stream of its own; False: torch's current stream
}


def main(config):
    import torch
    from promp_amd.envs.torch_point_env import TorchPointVecEnv
    np.random.seed(config['seed'])
    M = config['meta_batch_size']
    envs_per_task = config.get('envs_per_task') or config['rollouts_per_meta_task']
    env = MetaPointEnvV2()                             # draws the tasks (goals); the dynamics run in vec_env
    vec_env = TorchPointVecEnv(M, envs_per_task, stream=torch.cuda.Stream() if config.get('own_stream', True) else None)
    policy = MetaGaussianMLPPolicy(name='meta-policy', obs_dim=2, action_dim=2, meta_batch_size=M, hidden_sizes=config['hidden_sizes'])
    sampler = DeviceEnvSampler(vec_env, env, policy, rollouts_per_meta_task=config['rollouts_per_meta_task'], meta_batch_size=M,
                               max_path_length=config['max_path_length'], envs_per_task=envs_per_task,
                               poll_every=config.get('poll_every', 8))
    sample_processor = MetaSampleProcessor(baseline=LinearFeatureBaseline(), discount=config['discount'],
                                           gae_lambda=config['gae_lambda'], normalize_adv=config['normalize_adv'])
    algo = ProMP(policy=policy, inner_lr=config['inner_lr'], meta_batch_size=M,
                 num_inner_grad_steps=config['num_inner_grad_steps'], learning_rate=config['learning_rate'],
                 num_ppo_steps=config['num_promp_steps'], clip_eps=config['clip_eps'],
                 target_inner_step=config['target_inner_step'], init_inner_kl_penalty=config['init_inner_kl_penalty'],
                 adaptive_inner_kl_penalty=config['adaptive_inner_kl_penalty'])
    trainer = Trainer(algo=algo, policy=policy, env=env, sampler=sampler, sample_processor=sample_processor,
                      n_itr=config['n_itr'], num_inner_grad_steps=config['num_inner_grad_steps'])
    trainer.train()
    return policy


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description='ProMP on a torch environment that lives on the GPU (MI355X)')
    ap.add_argument('--config_file', type=str, default='')
    ap.add_argument('--dump_path', type=str, default='')
    ap.add_argument('--n_itr', type=int, default=None)
    ap.add_argument('--quiet', action='store_true')
    args = ap.parse_args()
    cfg = dict(DEFAULT)
    if args.config_file:
        cfg.update(json.load(open(args.config_file)))
    if args.n_itr is not None:
        cfg['n_itr'] = args.n_itr
    logger.configure(dir=args.dump_path or None, snapshot_mode='last_gap', snapshot_gap=50, quiet=args.quiet)
    if args.dump_path:
        json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, open(os.path.join(args.dump_path, 'params.json'), 'w'))
    main(cfg)
