// promp_objective.h -- the diagonal-Gaussian objective and its R-operator, once: the per-(row, action) arithmetic every policy-pass
// kernel shares (k_pass, k_chain_hvp, k_wide_*, k_wb_*, k_gen_loss), the row-level objective, and the FP16 cotangent scale.
// Plain force-inlined functions on scalars and small by-value structs: no template parameters of any family, no LDS, no lane ids.
// What differs between the families stays with them: masking of unowned actions / padding rows, the fold over a row's actions,
// where invN is multiplied in, signs and scales of the direction, stores.  Expression trees are the contract: the compiler
// contracts a * b + c after inlining, so a kernel's bits follow the association and operand order written here.
//
// Per action a of a row (new policy mu, s = log_std; old policy mo, so; sample ac):
//   z  = (ac - mu) e^{-s},  zo = (ac - mo) e^{-so}
//   log pi       = -sum_a (s + z^2 / 2) - (A / 2) log 2 pi           d log pi / dmu = z e^{-s},   d log pi / ds = z^2 - 1
//   log ratio    =  sum_a (so - s) - (z^2 - zo^2) / 2                 rho = exp(log ratio)
//   KL(old||new) =  sum_a num / den + s - so,   D = mo - mu,  num = D^2 + e^{2 so} - e^{2s},  den = 2 e^{2s} + 1e-8
//   dKL/dmu = -2 D / den                        dKL/ds = 1 - 2 P / den^2,  P = e^{2s} (den + 2 num)
//             (written as (-2 e^{2s} den - 4 num e^{2s}) / den^2 + 1)
// Row level: the objective's term lrow of the row, c = d lrow / d log pi, ck = the weight of the KL cotangents (LOSS_KL only):
//   LOSS_RATIO  -rho adv / N          c = -adv rho / N
//   LOSS_CLIP   -min(x, y) / N,  x = rho adv,  y = clip(rho, 1 -+ eps) adv;   c as LOSS_RATIO where x <= y, else 0
//   LOSS_LOGLIK -log pi adv / N       c = -adv / N
//   LOSS_KL      KL / N               c = 0,  ck = 1 / N
// so that d lrow / dmu = c z e^{-s} + ck dKL/dmu and d lrow / ds = c (z^2 - 1) + ck dKL/ds.
// R-operator (Pearlmutter) along a direction with tangents R'mu, R's of mu and s:
//   R'{log pi} = sum_a z e^{-s} R'mu + (z^2 - 1) R's           R'c = c R'{log pi} (LOSS_RATIO: c is proportional to rho), else 0
//   R'z = -R'mu e^{-s} - z R's
//   R'{c z e^{-s}}  = R'c z e^{-s} + c (R'z e^{-s} - z e^{-s} R's)
//   R'{c (z^2 - 1)} = R'c (z^2 - 1) + 2 c z R'z
// and when the objective is the mean KL itself (LOSS_KL, the TRPO constraint):
//   R'{dKL/dmu} = 2 R'mu / den + 8 D e^{2s} R's / den^2
//   R'{P}       = 2 e^{2s} R's (den + 2 num) - 4 e^{2s} D R'mu ;   R'{dKL/ds} = -2 R'{P} / den^2 + 16 P e^{2s} R's / den^3
#pragma once
#include "promp_device.h"

enum { LOSS_RATIO = 0, LOSS_CLIP = 1, LOSS_LOGLIK = 2, LOSS_KL = 3 };   // LOSS_KL: mean KL(old || new) itself (TRPO constraint)

// den of the KL term from sn2 = e^{2s}.  Its reciprocal `rden` is an argument below: every kernel produces it its own way
// (fast_rcp, once per task or per action; 1.0f / den in k_gen_loss), and so are the old policy's exponentials (per row or per task).
PROMP_DEV float gauss_kl_den(float sn2) { return 2.f * sn2 + 1e-8f; }

// The one-line pieces, for the lane-pair kernels that interleave their two actions; gauss_terms() is all of them for one action.
PROMP_DEV float gauss_z(float x, float m, float e) { return (x - m) * e; }
PROMP_DEV float gauss_log_ratio(float z, float zo, float s, float so) { return (so - s) - 0.5f * (z * z - zo * zo); }
PROMP_DEV float gauss_kl_num(float D, float sn2, float so2) { return D * D + so2 - sn2; }
PROMP_DEV float gauss_kl(float num, float rden, float s, float so) { return num * rden + s - so; }
struct GaussKlGrad { float dklm, dkls; };     // dKL/dmu, dKL/ds (without 1 / N)
PROMP_DEV GaussKlGrad gauss_kl_grad(float D, float sn2, float num, float den, float rden) {
    GaussKlGrad g;
    g.dklm = -2.f * D * rden;
    g.dkls = (-2.f * sn2 * den - 4.f * num * sn2) * (rden * rden) + 1.f;
    return g;
}
struct GaussTerms {
    float z, num, den;
    float dlp;                   // the action's term of the log ratio
    float kl, dklm, dkls;        // the action's term of the KL, its derivatives by mu and by s (without 1 / N)
};
PROMP_DEV GaussTerms gauss_terms(float ac, float mu, float s, float e, float sn2, float rden, float mo, float so, float eo, float so2) {
    GaussTerms g;
    g.z = gauss_z(ac, mu, e);
    g.dlp = gauss_log_ratio(g.z, gauss_z(ac, mo, eo), s, so);
    g.num = gauss_kl_num(mo - mu, sn2, so2);
    g.den = gauss_kl_den(sn2);
    g.kl = gauss_kl(g.num, rden, s, so);
    const GaussKlGrad k = gauss_kl_grad(mo - mu, sn2, g.num, g.den, rden);
    g.dklm = k.dklm;
    g.dkls = k.dkls;
    return g;
}

// the action's summand of R'{log pi}
PROMP_DEV float gauss_row_tangent(float z, float e, float Rmu, float Rs) { return z * e * Rmu + (z * z - 1.f) * Rs; }

// log-likelihood part: R'z, R'{c z e^{-s}} (mean cotangent), R'{c (z^2 - 1)} (log_std cotangent)
struct LikTangent { float Rz, Rd, Rds; };
PROMP_DEV LikTangent lik_tangent(float c, float Rc, float z, float e, float Rmu, float Rs) {
    LikTangent t;
    t.Rz = -Rmu * e - z * Rs;
    t.Rd = Rc * z * e + c * (t.Rz * e - z * e * Rs);
    t.Rds = Rc * (z * z - 1.f) + 2.f * c * z * t.Rz;
    return t;
}
// KL-objective part: R'{dKL/dmu}, R'{dKL/ds} (without 1 / N); D = mo - mu
struct KlTangent { float Rdm, Rds; };
PROMP_DEV KlTangent kl_tangent(float D, float sn2, float num, float den, float rden, float Rmu, float Rs) {
    const float P = sn2 * (den + 2.f * num);
    const float RP = 2.f * sn2 * Rs * (den + 2.f * num) - 4.f * sn2 * D * Rmu;
    KlTangent t;
    t.Rdm = 2.f * Rmu * rden + 8.f * D * sn2 * Rs * (rden * rden);
    t.Rds = (-2.f * RP + 16.f * P * sn2 * Rs * rden) * (rden * rden);
    return t;
}

// ---- row level.  sums = sum of the row's s, sumz2 = sum of its z^2.
PROMP_DEV float clip_x(float rho, float advn) { return rho * advn; }
PROMP_DEV float clip_y(float rho, float advn, float clip_eps) { return fminf(fmaxf(rho, 1.f - clip_eps), 1.f + clip_eps) * advn; }
PROMP_DEV float gauss_log_lik(float sums, float sumz2, int A) { return -sums - 0.5f * sumz2 - 0.5f * (float)A * 1.8378770664093453f; }

// The families round c and lrow in two orders; both are kept, each where it was.
struct RowObjective { float lrow, c, ck; };
// k_pass (and, spelled as assignments, k_gen_loss): the advantage's weight aw = adv / N first, then rho.  Branch free.
// km: the row's weight in ck (k_pass masks its padding rows there).
PROMP_DEV RowObjective row_objective_weight_first(int loss_kind, float rho, float kl, float advn, float invN, float km, float clip_eps,
                                                  float sums, float sumz2, int A) {
    const bool is_kl = loss_kind == LOSS_KL, is_ratio = loss_kind == LOSS_RATIO, is_clip = loss_kind == LOSS_CLIP;
    const float aw = advn * invN;
    const float x = clip_x(rho, advn), y = clip_y(rho, advn, clip_eps);
    const float lp = gauss_log_lik(sums, sumz2, A);
    RowObjective r;
    r.c = is_kl ? 0.f : is_ratio ? -aw * rho : is_clip ? ((x <= y) ? -aw * rho : 0.f) : -aw;
    r.ck = is_kl ? km * invN : 0.f;
    r.lrow = is_kl ? kl * invN : is_ratio ? -rho * aw : is_clip ? -fminf(x, y) * invN : -lp * aw;
    return r;
}
// k_wide_fwd_bwd, k_wb_fwd_bwd: adv rho first, 1 / N last.
PROMP_DEV RowObjective row_objective_invn_last(int loss_kind, float rho, float kl, float advn, float invN, float clip_eps,
                                               float sums, float sumz2, int A) {
    RowObjective r = {0.f, 0.f, 0.f};
    if (loss_kind == LOSS_KL) {
        r.lrow = kl * invN;
        r.ck = invN;
    } else if (loss_kind == LOSS_RATIO) {
        r.lrow = -rho * advn * invN;
        r.c = -advn * rho * invN;
    } else if (loss_kind == LOSS_CLIP) {
        const float x = clip_x(rho, advn), y = clip_y(rho, advn, clip_eps);
        r.lrow = -fminf(x, y) * invN;
        r.c = (x <= y) ? -advn * rho * invN : 0.f;
    } else {
        r.lrow = -gauss_log_lik(sums, sumz2, A) * advn * invN;
        r.c = -advn * invN;
    }
    return r;
}

// ---- log_std of one action as the policy uses it.  sr: the parameter (0 for an action slot past act_dim); with `clip` set the policy
// takes max(sr, min_s) (tf.maximum: the gradient passes where the parameter is at or above min_s, mask = 0 below it).
// Where the four terms go (LDS arrays, registers) and the direction's entry R's = mask v_s are the caller's business.  Users: k_wide_*,
// k_wb_* (coop_stage_log_std), k_gen_loss; chain_stage_dist (k_pass, k_chain_hvp) keeps the same lines in place, see there.
struct LogStdTerms {
    float s, es, sn2, mask;      // s, e^{-s}, e^{2s}, d s / d sr
    bool clipped;                // mask == 0, for the callers that select by it
};
PROMP_DEV LogStdTerms log_std_terms(float sr, int clip, float min_s) {
    LogStdTerms t;
    t.clipped = clip && (sr < min_s);
    t.s = t.clipped ? min_s : sr;
    t.es = expf(-t.s);
    t.sn2 = expf(2.f * t.s);
    t.mask = t.clipped ? 0.f : 1.f;
    return t;
}

// ---- FP16 split: the power of two 2^k a walk's cotangents are multiplied by (cs), its inverse (ics).  A largest |cotangent| of mx
// goes to [2^target, 2^(target + 1)); mx = 0 / not finite: 2^-4 N, for adv / N, and `prov` (no cotangent yet, the scale is still
// free).  The reasoning: promp_kernels_pass.h (PassSums).  Who reduces mx, over a wave or a workgroup, is the caller's business.
// scale_exp_clamped: the exponent k that takes |m| to [2^t, 2^(t + 1)), kept to +-100 so that 2^k and 2^-k are both normal floats; every
// scale of the split (the direction's, a walk's first and its redo's) is pow2f of it.
PROMP_DEV int scale_exp_clamped(float m, int t) {
    const int k = scale_exp(m, t);
    return k < -100 ? -100 : k > 100 ? 100 : k;
}
struct CotangentScale { float cs, ics; int prov; };
PROMP_DEV CotangentScale cotangent_scale(float mx, float invN, int target) {
    const bool okm = mx > 0.f && mx < 3.0e38f;
    const int k = scale_exp_clamped(okm ? mx : invN, okm ? target : -4);
    CotangentScale r;
    r.cs = pow2f(k);
    r.ics = pow2f(-k);
    r.prov = okm ? 0 : 1;
    return r;
}
