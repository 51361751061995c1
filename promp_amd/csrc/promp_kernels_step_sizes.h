// promp_kernels_step_sizes.h -- learned per-parameter inner step sizes (trainable_inner_step_size; the reference creates the
// variables, meta_algos/base.py:303-313, and never trains them, :203-211 -- this goes one step further: Meta-SGD, Li et al. 2017).
//
// Per task the inner chain is theta_{k+1} = theta_k - alpha * g_k and the backward sweep of the meta-gradient carries
// lam_k = dJ/dtheta_k.  The same objective's gradient with respect to alpha is
//     dJ/dalpha = sum_k  -lam_{k+1} * g_k        (elementwise; the inner-KL terms reach alpha only through theta_k)
// Both factors are already on the device: k_reduce_task (mode 0) keeps g_k next to theta_{k+1} (ReduceArgs::ginner), and lam
// holds the COMPLETE lam_{k+1} right in front of step k's R-operator pass -- for the DiCE inner objective too, whose two-piece
// reduction of step k + 1 has finished by then.  Nothing is recovered as (theta_k - theta_{k+1}) / alpha: step sizes may be zero.
//
//   k_step_size_grad : galpha[i] = (first ? 0 : galpha[i]) - lam[i] * g_k[i]        one launch per inner step, k = K-1 .. 0
//   PlainAdamRule / GeneralRule : one entry's step under tf.train.AdamOptimizer's defaults, or under the rule and arguments
//                      promp_set_outer_optimizer asked for (the plain and the general final-stage kernels of
//                      promp_kernels_policy.h: the same bodies over the rule type)
//   step_size_entry_step : that step on one alpha entry (behind the task sum of galpha)
#pragma once
#include "promp_device.h"
#include "promp_plan.h"            // OuterOptArgs

// grid = (ceil(NP / 256), tasks)
__global__ void __launch_bounds__(256) k_step_size_grad(float* galpha, const float* lam, const float* ginner, int NP, int first) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= NP) return;
    const long long tj = (long long)blockIdx.y * NP + j;
    const float acc = first ? 0.f : galpha[tj];
    galpha[tj] = acc - lam[tj] * ginner[tj];
}

// The outer rule of one entry's step, chosen at compile time: the plain final-stage kernels carry PlainAdamRule -- tf.train.
// AdamOptimizer's default constants as literals, no clip, no argument and no test at run time: a run-time branch in them is paid
// by every default step (profiles/step_size_timing.txt, profiles/outer_optimizer_timing.txt) --, the general ones GeneralRule.
// A rule gives Adam's constants, clipped(g) (the gradient the step takes) and step(): p the parameter, s1 / s2 its slots (Adam's
// m and v; Momentum's accumulator in s1), g the task-mean gradient after clipping, lr_t from outer_lr_t.
// Adam's lines, once; default arguments give the literals' bits in the same operation order.
template <class R>
PROMP_DEV void adam_entry_step(const R& r, float* p, float* s1, float* s2, int j, float g, float lr_t) {
    const float m = r.b1() * s1[j] + r.one_minus_b1() * g;
    const float v = r.b2() * s2[j] + r.one_minus_b2() * g * g;
    s1[j] = m;
    s2[j] = v;
    p[j] -= lr_t * m / (sqrtf(v) + r.eps());
}
struct PlainAdamRule {
    PROMP_DEV float b1() const { return 0.9f; }
    PROMP_DEV float one_minus_b1() const { return 0.1f; }
    PROMP_DEV float b2() const { return 0.999f; }
    PROMP_DEV float one_minus_b2() const { return 0.001f; }
    PROMP_DEV float eps() const { return 1e-8f; }
    PROMP_DEV float clipped(float g) const { return g; }
    PROMP_DEV void step(float* p, float* s1, float* s2, int j, float g, float lr_t) const { adam_entry_step(*this, p, s1, s2, j, g, lr_t); }
};
// Any rule and arguments of promp_set_outer_optimizer (include/promp_hip.h); scale the clip's factor, exactly 1 when the clip is
// off or not active.
struct GeneralRule {
    const OuterOptArgs& o;
    float scale;
    PROMP_DEV float b1() const { return o.b1; }
    PROMP_DEV float one_minus_b1() const { return o.one_minus_b1; }
    PROMP_DEV float b2() const { return o.b2; }
    PROMP_DEV float one_minus_b2() const { return o.one_minus_b2; }
    PROMP_DEV float eps() const { return o.eps; }
    PROMP_DEV float clipped(float g) const { return g * scale; }
    PROMP_DEV void step(float* p, float* s1, float* s2, int j, float g, float lr_t) const {
        if (o.rule == PROMP_OUTER_ADAM) {
            adam_entry_step(*this, p, s1, s2, j, g, lr_t);
        } else if (o.rule == PROMP_OUTER_SGD) {
            p[j] -= lr_t * g;
        } else {
            const float a = o.mu * s1[j] + g;
            s1[j] = a;
            p[j] -= lr_t * (o.nesterov ? g + o.mu * a : a);
        }
    }
};

// The rule's step on one step size with theta's arguments and lr_t (under plain Adam: what the reference's single minimize() would
// have done had its var_list held the step sizes); g unclipped.  An entry that is not trained (learn_std = False: the log_std
// entries) keeps its value and slots and reports no gradient.
template <class R>
PROMP_DEV void step_size_entry_step(const R& r, float* alpha, float* am, float* av, float* grad_mean, int j, float g, bool update,
                                    bool trained, float lr_t) {
    grad_mean[j] = trained ? g : 0.f;
    if (!update) return;
    r.step(alpha, am, av, j, r.clipped(g), lr_t);
}
