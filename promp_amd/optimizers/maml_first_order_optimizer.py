"""First-order optimisers of the MAML outer step: MAMLFirstOrderOptimizer, MAMLPPOOptimizer.

Behaviour contract (reference: meta_policy_search/optimizers/maml_first_order_optimizer.py:5-163; what ProMP and VPG-MAML call
through `self.optimizer`):

  * `optimize(inputs)` takes `max_epochs` full-batch steps of tf_optimizer_cls(**tf_optimizer_args) -- tf.train.AdamOptimizer(learning_rate)
    unless told otherwise -- on the meta-objective, the gradient clipped by its global norm first when `max_grad_norm` is set, and returns
    the loss BEFORE the first step (:82-115; `tolerance` is accepted and unused, as there, :97-113).  `num_minibatches` = B > 1 --
    documented there (:16-17) and left unimplemented (:41, :97-99) -- makes an epoch B Adam steps, one per minibatch: every task's
    paths of every sampling step are dealt to B shares (minibatch_assignment, drawn anew per epoch), minibatch j is the
    meta-objective on share j; the loss before and the statistics after stay whole-batch quantities (promp_optimize_minibatch);
  * `loss(inputs)` evaluates the meta-objective at the current parameters (:66-80);
  * MAMLPPOOptimizer.compute_stats(inputs) returns (loss, inner_kl [per inner step], outer_kl) at the current parameters (:146-163).

There is no graph to build here.  `build_graph` binds the optimiser to the algorithm plugin whose objective it steps (the reference
binds a loss tensor, a target policy and placeholders); every call is then one or more passes of the device kernels through the
plugin's DeviceSession: promp_optimize runs the E epochs AND the statistics pass behind them in one call, so `optimize` keeps what
the device handed back and a `compute_stats` / `loss` that follows it at unchanged parameters, data and coefficients answers from
there instead of walking the batch again (ProMP.optimize_policy asks exactly in that order, pro_mp.py:185-190).
"""
import numpy as np

from .. import _lib


def minibatch_assignment(path_counts, num_minibatches, rng=np.random):
    """The minibatch of every path of one sampling step: per task (path_counts: its number of paths, in task order) a permutation
    of its paths is drawn from `rng` (NumPy's global generator unless told otherwise: reproducible from np.random.seed, like the
    samplers), and the path of rank r among P goes to minibatch floor(r B / P) -- share sizes differ by at most one.
    -> int32 [sum(path_counts)], task after task.  A task with fewer paths than minibatches is refused."""
    B = int(num_minibatches)
    if B < 1:
        raise ValueError('num_minibatches must be >= 1, got %r' % (num_minibatches,))
    out = []
    for i, P in enumerate(int(p) for p in path_counts):
        if P < B:
            raise ValueError('num_minibatches = %d exceeds the %d paths of task %d' % (B, P, i))
        a = np.empty(P, dtype=np.int32)
        a[rng.permutation(P)] = (np.arange(P, dtype=np.int64) * B) // P
        out.append(a)
    return np.concatenate(out) if out else np.zeros(0, np.int32)


class Optimizer(object):
    """optimizers/base.py:3-36: the three calls an optimiser answers"""

    def build_graph(self, loss, target=None, input_ph_dict=None):
        raise NotImplementedError

    def optimize(self, input_val_dict=None):
        raise NotImplementedError

    def loss(self, input_val_dict=None):
        raise NotImplementedError


class MAMLFirstOrderOptimizer(Optimizer):
    """
    Args (maml_first_order_optimizer.py:22-46): tf_optimizer_cls -- None / 'adam', 'sgd' / 'gradient_descent', 'momentum', or a class
    named AdamOptimizer, GradientDescentOptimizer or MomentumOptimizer; anything else is refused by name (_lib.outer_rule_id) --,
    tf_optimizer_args -- beta1, beta2, epsilon (Adam), momentum, use_nesterov (Momentum), learning_rate; an unknown key is refused --,
    learning_rate, max_epochs, tolerance (unused), num_minibatches (steps per epoch, see above), verbose, max_grad_norm (None: no
    clipping; the reference has none).
    """

    def __init__(self, tf_optimizer_cls=None, tf_optimizer_args=None, learning_rate=1e-3, max_epochs=1, tolerance=1e-6,
                 num_minibatches=1, verbose=False, max_grad_norm=None):
        self._rule = _lib.outer_rule_id(tf_optimizer_cls)
        self._rule_args, lr = _lib.outer_rule_args(self._rule, tf_optimizer_args)
        self._max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._learning_rate = float(learning_rate if lr is None else lr)
        self._max_epochs = int(max_epochs)
        self._tolerance = tolerance
        self._num_minibatches = int(num_minibatches)
        if self._num_minibatches < 1:
            raise ValueError('num_minibatches must be >= 1, got %r' % (num_minibatches,))
        self._verbose = verbose
        self._algo = None
        self._memo = None                            # (key, result of the last promp_optimize)

    def build_graph(self, loss, target=None, input_ph_dict=None, **_):
        """`loss`: the algorithm plugin (a MAMLAlgo with a DeviceSession: .session, .inner_kind, .outer_kind and -- ProMP --
        .clip_eps, .inner_kl_coeff).  `target` / `input_ph_dict` are the reference's policy and placeholders: nothing to bind."""
        assert hasattr(loss, 'session'), 'build_graph binds the optimiser to an algorithm plugin (promp_amd.meta_algos.*)'
        loss.session.set_outer_optimizer(self._rule, self._rule_args, self._max_grad_norm)
        self._algo = loss
        self._memo = None

    # what the device evaluates with: the algorithm's current settings unless the call's dict overrides them (the reference feeds
    # clip_eps and the KL coefficients through the same dict as the samples, pro_mp.py:176-183)
    def _settings(self, input_val_dict):
        a, d = self._algo, (input_val_dict if isinstance(input_val_dict, dict) else {})
        K = a.num_inner_grad_steps
        clip_eps = float(d.get('clip_eps', getattr(a, 'clip_eps', 0.0)))
        eta = np.asarray(d.get('inner_kl_coeff', getattr(a, 'inner_kl_coeff', np.zeros(K))), dtype=np.float32).reshape(-1)
        return clip_eps, eta

    def _key(self, clip_eps, eta):
        # the context's own counter covers what param_version does not see: set_theta / set_step_sizes, advantages, min_std /
        # learn_std, trained step sizes (as _DeviceEvaluator._key, meta_algos/trpo_maml.py)
        s = self._algo.session
        ctx = s.ctx
        return (s.param_version, tuple(s.upload_serial), clip_eps, eta.tobytes(), self._algo.inner_kind, self._algo.outer_kind,
                id(ctx), None if ctx is None else ctx.state_version())

    def _place(self, input_val_dict):
        if isinstance(input_val_dict, (list, tuple)):          # all_samples_data: sampling step k into slot k
            self._algo._place_steps(input_val_dict)

    def optimize(self, input_val_dict=None):
        assert self._algo is not None, 'build_graph first'
        self._place(input_val_dict)
        clip_eps, eta = self._settings(input_val_dict)
        a = self._algo
        if self._num_minibatches > 1:
            res = self._optimize_minibatched(clip_eps, eta)
        else:
            res = a.session.optimize(self._max_epochs, self._learning_rate, clip_eps, eta, a.inner_kind, a.outer_kind)
        a.session.param_version += 1
        self._memo = (self._key(clip_eps, eta), res)
        return res['loss_before']

    def _optimize_minibatched(self, clip_eps, eta):
        """E epochs of B Adam steps: E x (K + 1) assignments, epoch after epoch and step after step, from np.random"""
        a = self._algo
        s = a.session
        if s.external():               # (refused there, with the reason, before anything is drawn)
            return s.optimize(self._max_epochs, self._learning_rate, clip_eps, eta, a.inner_kind, a.outer_kind,
                              num_minibatches=self._num_minibatches)
        ctx = s.ensure()
        counts = [np.diff(ctx.step_tpo[k]) for k in range(s.K + 1)]
        assign = [[minibatch_assignment(c, self._num_minibatches) for c in counts] for _ in range(self._max_epochs)]
        return s.optimize(self._max_epochs, self._learning_rate, clip_eps, eta, a.inner_kind, a.outer_kind,
                          num_minibatches=self._num_minibatches, assign=assign)

    def _evaluate(self, input_val_dict):
        assert self._algo is not None, 'build_graph first'
        self._place(input_val_dict)
        clip_eps, eta = self._settings(input_val_dict)
        key = self._key(clip_eps, eta)
        if self._memo is not None and self._memo[0] == key:
            r = self._memo[1]
            return dict(loss=r['loss_after'], inner_kl=r['inner_kl'], outer_kl=r['outer_kl'])
        a = self._algo
        r = a.session.meta_eval(clip_eps, eta, a.inner_kind, a.outer_kind)
        self._memo = (key, dict(loss_before=r['loss'], loss_after=r['loss'], inner_kl=r['inner_kl'], outer_kl=r['outer_kl']))
        return r

    def loss(self, input_val_dict=None):
        return self._evaluate(input_val_dict)['loss']

    @property
    def last_result(self):
        """what the last promp_optimize / evaluation returned: loss_before, loss_after, inner_kl, outer_kl"""
        return None if self._memo is None else self._memo[1]


class MAMLPPOOptimizer(MAMLFirstOrderOptimizer):
    """Adds the statistics of the PPO-style outer objective (maml_first_order_optimizer.py:118-163)"""

    def build_graph(self, loss, target=None, input_ph_dict=None, inner_kl=None, outer_kl=None, **_):
        super(MAMLPPOOptimizer, self).build_graph(loss, target, input_ph_dict)

    def compute_stats(self, input_val_dict=None):
        r = self._evaluate(input_val_dict)
        return r['loss'], r['inner_kl'], r['outer_kl']


__all__ = ['Optimizer', 'MAMLFirstOrderOptimizer', 'MAMLPPOOptimizer', 'minibatch_assignment']
_ = _lib      # (the kinds the plugins carry are _lib's INNER_* / OUTER_* constants)
