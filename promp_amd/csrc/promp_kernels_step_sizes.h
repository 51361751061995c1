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
//   step_size_adam   : the Adam step of one alpha entry (k_mean_adam / k_final_adam, behind the task sum of galpha)
//   outer_rule_step  : one entry's step under the rule promp_set_outer_optimizer asked for (the general final-stage kernels
//                      k_mean_outer / k_final_outer of promp_kernels_policy.h: theta's entries and, step_size_outer, alpha's)
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

// tf.train.AdamOptimizer on one step size with theta's beta_1, beta_2, epsilon and bias-corrected lr_t (what the reference's
// single minimize() would have done had its var_list held the step sizes); an entry that is not trained (learn_std = False:
// the log_std entries) keeps its value and slots and reports no gradient
PROMP_DEV void step_size_adam(float* alpha, float* am, float* av, float* grad_mean, int j, float g, bool update, bool trained,
                              float lr_t) {
    grad_mean[j] = trained ? g : 0.f;
    if (!update) return;
    const float m = 0.9f * am[j] + 0.1f * g;
    const float v = 0.999f * av[j] + 0.001f * g * g;
    am[j] = m;
    av[j] = v;
    alpha[j] -= lr_t * m / (sqrtf(v) + 1e-8f);
}

// One entry's step under any rule (include/promp_hip.h, promp_set_outer_optimizer): p the parameter, s1 / s2 its slots (Adam's m
// and v; Momentum's accumulator in s1), g the task-mean gradient after clipping, lr_t from outer_lr_t.  The Adam lines are the
// plain kernels' lines with the constants as arguments, in the same operation order: default arguments give the same bits.
PROMP_DEV void outer_rule_step(const OuterOptArgs& o, float* p, float* s1, float* s2, int j, float g, float lr_t) {
    if (o.rule == PROMP_OUTER_ADAM) {
        const float m = o.b1 * s1[j] + o.one_minus_b1 * g;
        const float v = o.b2 * s2[j] + o.one_minus_b2 * g * g;
        s1[j] = m;
        s2[j] = v;
        p[j] -= lr_t * m / (sqrtf(v) + o.eps);
    } else if (o.rule == PROMP_OUTER_SGD) {
        p[j] -= lr_t * g;
    } else {
        const float a = o.mu * s1[j] + g;
        s1[j] = a;
        p[j] -= lr_t * (o.nesterov ? g + o.mu * a : a);
    }
}
// step_size_adam under any rule; g unclipped, scale the clip's factor (exactly 1 when it is off or not active)
PROMP_DEV void step_size_outer(const OuterOptArgs& o, float* alpha, float* am, float* av, float* grad_mean, int j, float g, float scale,
                               bool update, bool trained, float lr_t) {
    grad_mean[j] = trained ? g : 0.f;
    if (!update) return;
    outer_rule_step(o, alpha, am, av, j, g * scale, lr_t);
}
