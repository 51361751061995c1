#!/usr/bin/env python
"""DICE-MAML / VPG-DICE-MAML on the 2-D point-mass meta-environment -- the promp_amd counterpart of the reference's DiCE run
scripts (same config keys), with the environment, the sample processing and the meta-step all on the device:
DevicePointEnvSampler -> DiceMetaSampleProcessor -> DICEMAML (--vpg: VPG_DICEMAML, whose processor has a return baseline).

    python run_scripts/dice_maml_run_point_mass.py [--vpg] [--config_file cfg.json] [--dump_path DIR] [--n_itr N]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from promp_amd.baselines.linear_baseline import LinearFeatureBaseline, LinearTimeBaseline  # noqa: E402
from promp_amd.envs.normalized_env import normalize  # noqa: E402
from promp_amd.envs.point_env import make_point_env  # noqa: E402
from promp_amd.meta_algos.dice_maml import DICEMAML  # noqa: E402
from promp_amd.meta_algos.vpg_dice_maml import VPG_DICEMAML  # noqa: E402
from promp_amd.meta_trainer import Trainer  # noqa: E402
from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy  # noqa: E402
from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler  # noqa: E402
from promp_amd.samplers.dice_sample_processor import DiceMetaSampleProcessor  # noqa: E402
from promp_amd.samplers.meta_sampler import MetaSampler  # noqa: E402
from promp_amd.utils import logger  # noqa: E402

DEFAULT = {
    'seed': 1, 'baseline': 'LinearTimeBaseline', 'env': 'MetaPointEnvCorner', 'reward_type': 'sparse', 'normalize_env': True,
    'rollouts_per_meta_task': 20, 'max_path_length': 100, 'parallel': False,
    'discount': 0.99, 'gae_lambda': 1, 'normalize_adv': True, 'positive_adv': False,
    'hidden_sizes': (32, 32),
    'inner_lr': 0.1, 'learning_rate': 1e-3,
    'n_itr': 100, 'meta_batch_size': 4, 'num_inner_grad_steps': 1,
    'vpg': False,                  # True: VPG_DICEMAML (DiCE inner steps, vanilla policy gradient outside) with a return baseline
    'device_rollouts': True,       # False: MetaSampler on the host (the processor then uploads each batch once)
    'device_noise': False,
    'device_starts': False,        # every reset() drawn on the device (Philox); no start table is built or uploaded
}

BASELINES = {'LinearFeatureBaseline': LinearFeatureBaseline, 'LinearTimeBaseline': LinearTimeBaseline}


def main(config):
    np.random.seed(config['seed'])
    env = make_point_env(config.get('env', 'corner'), config.get('reward_type', 'sparse'))
    if config.get('normalize_env', True):
        env = normalize(env, normalize_obs=bool(config.get('normalize_obs', False)), normalize_reward=bool(config.get('normalize_reward', False)),
                        obs_alpha=config.get('obs_alpha', 0.001), reward_alpha=config.get('reward_alpha', 0.001))
    policy = MetaGaussianMLPPolicy(name='meta-policy', obs_dim=int(np.prod(env.observation_space.shape)), action_dim=2,
                                   meta_batch_size=config['meta_batch_size'],
                                   hidden_sizes=config['hidden_sizes'])
    sampler_kwargs = dict(env=env, policy=policy, rollouts_per_meta_task=config['rollouts_per_meta_task'],
                          meta_batch_size=config['meta_batch_size'], max_path_length=config['max_path_length'],
                          parallel=config['parallel'])
    if config.get('device_rollouts', True):
        sampler = DevicePointEnvSampler(device_noise=bool(config.get('device_noise')), device_starts=bool(config.get('device_starts')),
                                        **sampler_kwargs)
    else:
        sampler = MetaSampler(**sampler_kwargs)
    extra = dict(return_baseline=LinearFeatureBaseline()) if config.get('vpg') else {}
    sample_processor = DiceMetaSampleProcessor(baseline=BASELINES[config['baseline']](), max_path_length=config['max_path_length'],
                                               discount=config['discount'], gae_lambda=config['gae_lambda'],
                                               normalize_adv=config['normalize_adv'], positive_adv=config['positive_adv'], **extra)
    algo_cls = VPG_DICEMAML if config.get('vpg') else DICEMAML
    algo = algo_cls(config['max_path_length'], policy=policy, inner_lr=config['inner_lr'], meta_batch_size=config['meta_batch_size'],
                    num_inner_grad_steps=config['num_inner_grad_steps'], learning_rate=config['learning_rate'])
    trainer = Trainer(algo=algo, policy=policy, env=env, sampler=sampler, sample_processor=sample_processor,
                      n_itr=config['n_itr'], num_inner_grad_steps=config['num_inner_grad_steps'])
    trainer.train()
    return policy


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description='DICE-MAML / VPG-DICE-MAML on the point mass (MI355X)')
    ap.add_argument('--config_file', type=str, default='')
    ap.add_argument('--dump_path', type=str, default='')
    ap.add_argument('--n_itr', type=int, default=None)
    ap.add_argument('--env', type=str, default=None, choices=['corner', 'walls', 'momentum', 'origin', 'goal'],
                    help='the point-mass meta-environment (default corner); walls and momentum take their own default reward type '
                         'unless the config file names one; origin (MetaPointEnv) and goal (MetaPointEnvV2) end their episodes '
                         'early and have no reward type')
    ap.add_argument('--vpg', action='store_true', help='VPG_DICEMAML: DiCE inner steps, advantages from a return baseline outside')
    ap.add_argument('--normalize_obs', action='store_true',
                    help='the normalize wrapper\'s running observation normalisation (with device_rollouts: device-resident moments)')
    ap.add_argument('--normalize_reward', action='store_true', help='the normalize wrapper\'s running reward normalisation')
    ap.add_argument('--obs_alpha', type=float, default=None, help='step size of the running observation moments (default 0.001)')
    ap.add_argument('--reward_alpha', type=float, default=None, help='step size of the running reward moments (default 0.001)')
    ap.add_argument('--device_starts', action='store_true',
                    help='with device_rollouts: start states drawn on the device instead of NumPy\'s RNG (use with device_noise)')
    ap.add_argument('--quiet', action='store_true')
    args = ap.parse_args()
    cfg = dict(DEFAULT)
    if args.config_file:
        cfg.update(json.load(open(args.config_file)))
    if args.env is not None:
        cfg['env'] = args.env
        if not (args.config_file and 'reward_type' in json.load(open(args.config_file))):
            cfg['reward_type'] = None          # the class's default
    if args.n_itr is not None:
        cfg['n_itr'] = args.n_itr
    if args.vpg:
        cfg['vpg'] = True
    for key in ('normalize_obs', 'normalize_reward', 'device_starts'):
        if getattr(args, key):
            cfg[key] = True
    for key in ('obs_alpha', 'reward_alpha'):
        if getattr(args, key) is not None:
            cfg[key] = getattr(args, key)
    logger.configure(dir=args.dump_path or None, snapshot_mode='last_gap', snapshot_gap=50, quiet=args.quiet)
    if args.dump_path:
        json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, open(os.path.join(args.dump_path, 'params.json'), 'w'))
    main(cfg)
