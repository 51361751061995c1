"""MAMLAlgo (reference: meta_policy_search/meta_algos/base.py:88-313): inner adaptation step and the
bookkeeping that maps processed samples onto device-resident slabs."""
import numpy as np

from .. import _lib
from ..utils import logger


class MetaAlgo(object):
    def __init__(self, policy):
        assert hasattr(policy, 'session') and hasattr(policy, 'update_task_parameters')
        self.policy = policy
        self._optimization_keys = None


class MAMLAlgo(MetaAlgo):
    """
    Args (meta_algos/base.py:100-113): policy, inner_lr=0.1, meta_batch_size=20, num_inner_grad_steps=1,
    trainable_inner_step_size=False
    """
    inner_kind = _lib.INNER_RATIO
    trains_step_sizes = True      # trainable_inner_step_size is honoured (TRPOMAML: its step is over theta alone)

    def __init__(self, policy, inner_lr=0.1, meta_batch_size=20, num_inner_grad_steps=1, trainable_inner_step_size=False):
        super(MAMLAlgo, self).__init__(policy)
        assert type(num_inner_grad_steps) and num_inner_grad_steps >= 0
        assert type(meta_batch_size) == int
        assert meta_batch_size == policy.meta_batch_size
        self.inner_lr = float(inner_lr)
        self.meta_batch_size = meta_batch_size
        self.num_inner_grad_steps = num_inner_grad_steps
        # The reference creates the step-size variables with trainable=... (base.py:303-313) and then leaves them out of its
        # optimiser's var_list (base.py:203, maml_first_order_optimizer.py:64): there the flag changes nothing.  Here True trains
        # them: the outer Adam steps update one step size per parameter together with theta (Meta-SGD).
        self.trainable_inner_step_size = bool(trainable_inner_step_size)
        self.session = policy.session
        self.session.set_num_inner_steps(num_inner_grad_steps)
        # per-parameter step-size tensors initialised to inner_lr (base.py:303-313)
        self.session.set_step_sizes(np.full(self.session.theta.size, self.inner_lr, dtype=np.float32))
        self.session.set_train_step_sizes(self.trainable_inner_step_size and self.trains_step_sizes)
        self._adapt_count = 0

    @property
    def step_sizes(self):
        """[Theta] inner step sizes: np.full(Theta, inner_lr) unless trainable_inner_step_size moves them"""
        return self.session.get_step_sizes()

    def _init_outer_optimizer(self, tf_optimizer_cls=None, tf_optimizer_args=None, max_grad_norm=None):
        """the rule of the outer step, its arguments and the gradient clip (MAMLFirstOrderOptimizer's arguments, which the
        reference's algorithms do not pass on) -> the session; a learning_rate among the arguments replaces the algorithm's"""
        rule = _lib.outer_rule_id(tf_optimizer_cls)
        args, lr = _lib.outer_rule_args(rule, tf_optimizer_args)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.session.set_outer_optimizer(rule, args, self.max_grad_norm)
        if lr is not None:
            self.learning_rate = lr

    def _log_grad_norm(self):
        if getattr(self, 'max_grad_norm', None):
            logger.logkv('GradNorm', self.session.grad_norm())

    def _log_step_sizes(self):
        if self.session.train_step_sizes:
            s = self.step_sizes
            logger.logkv('InnerStepSize-Mean', float(np.mean(s)))
            logger.logkv('InnerStepSize-Min', float(np.min(s)))
            logger.logkv('InnerStepSize-Max', float(np.max(s)))

    def _slot_of(self, samples, default_slot):
        """device slot that holds `samples` (uploading them if they did not come from our sample processor)"""
        slot = self.session.resident_slot(samples)
        if slot is None:
            slot = default_slot % (self.num_inner_grad_steps + 1)
            self._upload_into(slot, samples)
        return slot

    def _place_steps(self, all_samples_data):
        """sampling step k into slot k for every k.  The context is sized for the largest step that has to be uploaded BEFORE
        the first upload: a context that grows between two uploads would drop the slabs uploaded so far."""
        missing = [sd for k, sd in enumerate(all_samples_data) if self.session.resident_slot(sd) != k]
        if missing:
            n_paths = lambda sd: sum(len(d['path_lengths']) if 'path_lengths' in d else 1 for d in sd)
            self.session.ensure(max(sum(len(d['advantages']) for d in sd) for sd in missing), max(n_paths(sd) for sd in missing))
        for k, sd in enumerate(all_samples_data):
            if self.session.resident_slot(sd) != k:   # not resident, or resident in another slot (an extra process_samples call)
                self._upload_into(k, sd)

    def _upload_into(self, slot, samples):
        """host copy of `samples` -> `slot`; the samples remember where they now live, so the next call finds them resident
        instead of uploading again (and instead of displacing the step that owns the slot they used to point at)"""
        upload = self.session.upload_samples(slot, samples)
        for i, sd in enumerate(samples):
            if hasattr(sd, 'device_ref'):
                sd.device_ref = (self.session.serial, upload, slot, i)

    def _adapt(self, samples):
        """MAML inner step for each task; stores the adapted parameters in the policy (base.py:217-242)"""
        assert len(samples) == self.meta_batch_size
        if self.policy._pre_update_mode:
            self._adapt_count = 0
        slot = self._slot_of(samples, self._adapt_count)
        self.session.ensure()
        self.session.ctx.inner_adapt(slot, self.inner_kind)
        self._adapt_count += 1
        self.session.task_thetas = None
        self.session.param_version += 1
        self.policy._pre_update_mode = False
