"""MetaPointEnvV2's dynamics as a vectorised environment on torch tensors that live on the GPU: an example of the vec_env protocol
of samplers/device_env_sampler.py, and its test vehicle.

    reset: state = (0, 0);  step: s' = s + clip(action, -0.1, 0.1);  reward -|goal - s'|;
    done: |s'_0| < 0.01 and |s'_1| < 0.01 -- the box around the origin, as envs/point_env.py:MetaPointEnvV2 has it

State and arithmetic are float64, observations float32, as the NumPy class handed to a float32 policy.  This is an example of an
environment the library has never seen, not a restatement of the built-in goal kind (promp_collect_point_family): torch's kernels
round the norm as they please, so no parity with it is claimed.

torch is imported by this module alone; the package does not depend on it.  Everything is enqueued on `stream` (default: torch's
current stream at construction), which DeviceEnvSampler hands to the library for ordering; no call here synchronises.
"""
import numpy as np
import torch

DONE_RADIUS = 0.01
MAX_STEP = 0.1


class TorchPointVecEnv(object):
    def __init__(self, meta_batch_size, envs_per_task, device='cuda', stream=None):
        self.meta_batch_size, self.envs_per_task = int(meta_batch_size), int(envs_per_task)
        self.n_envs = self.meta_batch_size * self.envs_per_task
        self.device = torch.device(device)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self.stream):
            self.state = torch.zeros((self.n_envs, 2), dtype=torch.float64, device=self.device)
            self.goals = torch.zeros((self.n_envs, 2), dtype=torch.float64, device=self.device)
            self.obs = torch.zeros((self.n_envs, 2), dtype=torch.float32, device=self.device)
            self.rewards = torch.zeros(self.n_envs, dtype=torch.float32, device=self.device)
            self.done = torch.zeros(self.n_envs, dtype=torch.uint8, device=self.device)

    # ---- the tasks: what MetaPointEnvV2.sample_tasks draws ----
    @staticmethod
    def sample_tasks(n_tasks):
        return np.random.uniform(-2, 2, size=(n_tasks, 2))

    def set_tasks(self, tasks):
        goals = np.repeat(np.asarray(tasks, dtype=np.float64).reshape(self.meta_batch_size, 2), self.envs_per_task, axis=0)
        with torch.cuda.stream(self.stream):
            self.goals.copy_(torch.from_numpy(goals))

    def empty(self, shape, dtype):
        """the sampler's `actions` and `ended` as tensors of this environment's device"""
        with torch.cuda.stream(self.stream):
            return torch.zeros(tuple(shape), dtype={'float32': torch.float32, 'uint8': torch.uint8}[np.dtype(dtype).name], device=self.device)

    # ---- the protocol ----
    def reset(self):
        with torch.cuda.stream(self.stream):
            self.state.zero_()
            self.obs.copy_(self.state)
        return self.obs

    def step(self, actions):
        with torch.cuda.stream(self.stream):
            move = torch.clamp(actions.to(torch.float64), -MAX_STEP, MAX_STEP)
            self.state.add_(move)
            self.rewards.copy_(-torch.linalg.vector_norm(self.goals - self.state, dim=1))
            self.done.copy_((self.state.abs() < DONE_RADIUS).all(dim=1))
            self.obs.copy_(self.state)
        return self.obs, self.rewards, self.done

    def reset_where(self, ended):
        with torch.cuda.stream(self.stream):
            self.state.mul_((ended == 0).to(torch.float64).unsqueeze(1))     # (MetaPointEnvV2.reset: back to the origin)
            self.obs.copy_(self.state)
        return self.obs
