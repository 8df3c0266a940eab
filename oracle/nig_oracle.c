/*
 * nig_oracle.c -- TEST INFRASTRUCTURE ONLY.  Not part of the product.
 *
 * A scalar, plain-C CPU restatement of the reference's NumPy hot path
 * (danieleschmidt/neoRL-industrial-gym, IndustrialEnv.step / reset and the three
 * working environments).  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may load this library; the product (libnig.so) never does.
 *
 * Parity pin: checked bit-for-bit / within 1e-5 against golden vectors produced by
 * RUNNING the reference in the build container (oracle/gen_golden.py ->
 * tests/golden/ (npz); NumPy 2.2.6 semantics, float32 actions).  See
 * tests/test_oracle_golden.py.
 *
 * Every function cites the reference file:line it follows (paths relative to
 * /root/reference/src/neorl_industrial/).  Arithmetic notes (NEP-50 weak scalars,
 * Python min/max first-argument-wins, NumPy pairwise 8-sum) are from SURVEY.md
 * Appendix A and were re-verified against the goldens.
 *
 * Build: see oracle/Makefile  (gcc -O2 -ffp-contract=off, no fast-math).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORACLE_CR 0
#define ORACLE_PG 1
#define ORACLE_RA 2
#define ORACLE_ACR 3 /* AdvancedChemicalReactor-v0: candidate row, no upstream output exists (not instantiable) */
#define ORACLE_APG 4 /* AdvancedPowerGrid-v0: same */
/* 5..8: HVACControl / WaterTreatment / SteelAnnealing / SupplyChain -- BUILD-SPECIFIED plants: the reference's
 * README names them (README.md:28-32) and ships no implementation, so this file is not an oracle OF THE
 * REFERENCE for them, only the independent CPU statement the device code is checked against. */
#define ORACLE_SPEC0 5
#define ORACLE_NUM_ENVS 9

#define MATH_LIBM 0 /* libm expf / sin / cos                    */
#define MATH_POLY 1 /* documented polynomials (DESIGN.md "detmath"), bitwise = device */

/* ------------------------------------------------------------------------------
 * detmath: polynomial exp/log/sincos/pow/tanh written ONLY with IEEE + - * / and explicit fma (no
 * libm, no compiler contraction) so that a CPU and a GPU evaluation agree bit-for-bit.  Specification in
 * DESIGN.md section "Deterministic math".  Coefficients are the classic Cephes
 * single-precision / fdlibm double-precision minimax sets.
 * ---------------------------------------------------------------------------- */
static float det_expf(float x)
{
    if (x != x) return x;
    if (x > 88.72283f) return INFINITY;
    if (x < -103.0f) return 0.0f;
    float fk = floorf(fmaf(x, 1.44269504088896341f, 0.5f));
    float r = fmaf(-fk, 0.693359375f, x);
    r = fmaf(-fk, -2.12194440e-4f, r);
    float z = r * r;
    float p = 1.9875691500e-4f;
    p = fmaf(p, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    p = fmaf(p, z, r);
    p = p + 1.0f;
    int k = (int)fk;
    /* scale by 2^k in two exact steps so that subnormal results round once */
    int k1 = k / 2, k2 = k - k1;
    union { uint32_t u; float f; } s1, s2;
    s1.u = (uint32_t)(k1 + 127) << 23;
    s2.u = (uint32_t)(k2 + 127) << 23;
    return (p * s1.f) * s2.f;
}

/* natural log of a float in (0, 1] (normal numbers only; callers pass k*2^-24, k>=1) */
static float det_logf(float x)
{
    union { float f; uint32_t u; } v; v.f = x;
    int e = (int)(v.u >> 23) - 126;                  /* x = m * 2^e, m in [0.5,1) */
    v.u = (v.u & 0x007fffffu) | 0x3f000000u;
    float m = v.f;
    if (m < 0.707106781186547524f) { e -= 1; m = m + m - 1.0f; } else { m = m - 1.0f; }
    float z = m * m;
    float y = 7.0376836292e-2f;
    y = y * m + -1.1514610310e-1f;
    y = y * m + 1.1676998740e-1f;
    y = y * m + -1.2420140846e-1f;
    y = y * m + 1.4249322787e-1f;
    y = y * m + -1.6668057665e-1f;
    y = y * m + 2.0000714765e-1f;
    y = y * m + -2.4999993993e-1f;
    y = y * m + 3.3333331174e-1f;
    y = y * m * z;
    float fe = (float)e;
    y = y + -2.12194440e-4f * fe;
    y = y + -0.5f * z;
    float r = m + y;
    r = r + 0.693359375f * fe;
    return r;
}

/* double sin/cos for moderate |x| (joint angles, |x| <= ~1e3): Cody-Waite + fdlibm kernels */
static void det_sincos(double x, double *s, double *c)
{
    double fk = floor(fma(x, 0.63661977236758134308, 0.5));
    double r = fma(-fk, 1.57079632673412561417e+00, x);
    r = fma(-fk, 6.07710050650619224932e-11, r);
    double z = r * r;
    double ps = 1.58969099521155010221e-10;
    ps = fma(ps, z, -2.50507602534068634195e-08);
    ps = fma(ps, z, 2.75573137070700676789e-06);
    ps = fma(ps, z, -1.98412698298579493134e-04);
    ps = fma(ps, z, 8.33333333332248946124e-03);
    ps = fma(ps, z, -1.66666666666666324348e-01);
    double sn = fma(r * z, ps, r);
    double pc = -1.13596475577881948265e-11;
    pc = fma(pc, z, 2.08757232129817482790e-09);
    pc = fma(pc, z, -2.75573143513906633035e-07);
    pc = fma(pc, z, 2.48015872894767294178e-05);
    pc = fma(pc, z, -1.38888888888741095749e-03);
    pc = fma(pc, z, 4.16666666666666019037e-02);
    double cs = fma(z * z, pc, fma(-0.5, z, 1.0));
    /* quadrant = fk mod 4, read from the low mantissa bits of fk + 1.5 * 2^52 (the two's complement of fk for
     * |fk| < 2^51, i.e. everywhere the two-constant reduction above means anything; defined, unlike a cast, for every
     * other double as well): the statement the device code uses, so that the two agree on ALL inputs */
    double km = fk + 6755399441055744.0;
    uint64_t kb;
    memcpy(&kb, &km, sizeof kb);
    uint32_t q = (uint32_t)kb;
    switch ((int)(q & 3u)) {
    case 0: *s = sn;  *c = cs;  break;
    case 1: *s = cs;  *c = -sn; break;
    case 2: *s = -sn; *c = -cs; break;
    default: *s = -cs; *c = sn; break;
    }
}

static float det_powf(float x, float y) { return (x > 0.0f) ? det_expf(y * det_logf(x)) : 0.0f; }
/* tanh: Cephes tanhf's odd degree-9 polynomial below |x| = 0.625, (1 - e^-2|x|) / (1 + e^-2|x|) above, sign of x copied */
static float det_tanhf(float x)
{
    float ax = fabsf(x);
    if (!(ax < 0.625f)) {
        float e = det_expf(-2.0f * ax);
        return copysignf((1.0f - e) / (1.0f + e), x);
    }
    float z = ax * ax;
    float p = -5.70498872745e-3f;
    p = fmaf(p, z, 2.06390887954e-2f);
    p = fmaf(p, z, -5.37397155531e-2f);
    p = fmaf(p, z, 1.33314422036e-1f);
    p = fmaf(p, z, -3.33332819422e-1f);
    return copysignf(fmaf(p * z, ax, ax), x);
}
/* logistic sigmoid, the safety critic's output (agents/cql.py predict_with_safety) */
static float det_sigmoidf(float x) { return 1.0f / (1.0f + det_expf(-x)); }
static float det_sinf(float x)
{
    float fk = floorf(x * 0.636619772367581343f + 0.5f);
    float r = x - fk * 1.5703125f;
    r = r - fk * 4.837512969970703125e-4f;
    r = r - fk * 7.54978995489188216e-8f;
    float z = r * r;
    float sp = -1.9515295891e-4f;
    sp = sp * z + 8.3321608736e-3f;
    sp = sp * z + -1.6666654611e-1f;
    sp = sp * z * r + r;
    float cp = 2.443315711809948e-5f;
    cp = cp * z + -1.388731625493765e-3f;
    cp = cp * z + 4.166664568298827e-2f;
    cp = cp * z * z;
    cp = cp + -0.5f * z;
    cp = cp + 1.0f;
    /* quadrant from the low mantissa bits of fk + 1.5 * 2^23 (fk mod 4 for |fk| < 2^22; defined for every float,
     * unlike a float -> int conversion): the statement the device uses */
    union { float f; uint32_t u; } km; km.f = fk + 12582912.0f;
    uint32_t q = km.u;
    float v = (q & 1u) ? cp : sp;
    return (q & 2u) ? -v : v;
}
static float o_powf(float x, float y, int flavor) { return flavor == MATH_POLY ? det_powf(x, y) : powf(x, y); }
static float o_tanhf(float x, int flavor) { return flavor == MATH_POLY ? det_tanhf(x) : tanhf(x); }
static float o_sinf(float x, int flavor) { return flavor == MATH_POLY ? det_sinf(x) : sinf(x); }

static float o_expf(float x, int flavor) { return flavor == MATH_POLY ? det_expf(x) : expf(x); }
static void o_sincos(double x, int flavor, double *s, double *c)
{
    if (flavor == MATH_POLY) { det_sincos(x, s, c); } else { *s = sin(x); *c = cos(x); }
}

/* Python's builtin max(a, b) / min(a, b): "b if b > a else a" / "b if b < a else a"
 * (first argument wins ties and NaNs).  Used wherever the reference calls builtin
 * min/max on scalars, e.g. chemical_reactor.py:166-167,175-176,186-187,195,216. */
static float pymaxf(float a, float b) { return (b > a) ? b : a; }
static float pyminf(float a, float b) { return (b < a) ? b : a; }
static double pymaxd(double a, double b) { return (b > a) ? b : a; }
static double pymind(double a, double b) { return (b < a) ? b : a; }

/* NumPy add.reduce over exactly 8 contiguous elements: 8 accumulators then the tree
 * ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))  (numpy pairwise_sum, n == 8). */
static float sum8f(const float *x) { return ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7])); }
static double sum8d(const double *x) { return ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7])); }

/* ------------------------------------------------------------------------------
 * environment tables  (base.py:22-72 ctor; per-env ctor constants)
 * ---------------------------------------------------------------------------- */
typedef struct {
    int state_dim, action_dim, n_constraints;
    int k_step, k_reset;          /* RNG draws per step / per reset, in reference call order */
    int max_episode_steps;        /* default */
    double dt;                    /* default */
    double penalty[3];
    int critical[3];
} oracle_spec_t;

static oracle_spec_t SPECS[ORACLE_NUM_ENVS] = {
    /* chemical_reactor.py:38-69 */ {12, 3, 3, 2, 8, 500, 0.1, {-100.0, -50.0, -25.0}, {1, 1, 0}},
    /* power_grid.py:53-79       */ {32, 8, 3, 23, 31, 1000, 0.1, {-50.0, -30.0, -20.0}, {1, 1, 0}},
    /* robot_assembly.py:56-82   */ {24, 7, 3, 0, 7, 1000, 0.1, {-100.0, -200.0, -50.0}, {1, 1, 0}},
    /* advanced_chemical_reactor.py:50-62,109-115 (dt: base.py:44 overwrites the 1.0 of :65) */
    {20, 6, 4, 0, 0, 1000, 0.1, {0.0, 0.0, 0.0}, {0, 0, 0}},
    /* advanced_power_grid.py:55-63,124-130 */ {32, 8, 3, 0, 0, 500, 0.1, {0.0, 0.0, 0.0}, {0, 0, 0}},
};

/* ------------------------------------------------------------------------------
 * Build-specified plants (model: neorl-industrial-gym_amd/spec_plants.py, the generator of the
 * table data compiled here).  State = [y_0..y_np-1, p_0..p_na-1, e, E, t]; float32, fixed order, one rounding
 * per operation where a multiply-add is ONE operation (model arithmetic "v2": fmaf here, v_fma_f32 on the device).
 * ---------------------------------------------------------------------------- */
#include "nig_spec_plants.inc"
typedef struct {
    int np, na;
    float y0[15], sd0[15], k[15], amb[15], cpl[15];
    int cidx[15];
    float ymin[15], ymax[15], sp[15], w[15];
    float G[15][10];
    float rate[10], ecost[10];
    float nsd[2];
    float we, wu, bonus;
    int cfirst[3], ccount[3];
    float clo[3], chi[3], pen[3];
    int crit[3];
    int d_idx;
    float dlo, dhi;
} spec_plant_t;
static const spec_plant_t SPEC_PLANTS[4] = {NIG_SPEC_PLANT_ROWS};
static const int SPEC_MAXSTEPS[4] = {NIG_SPEC_MAXSTEPS_LIST};

static int sp_box_ok(const spec_plant_t *P, int c, const float *s)
{
    int ok = 1;
    for (int r = P->cfirst[c]; r < P->cfirst[c] + P->ccount[c]; r++) ok = ok && (P->clo[c] <= s[r]) && (s[r] <= P->chi[c]);
    return ok;
}
static void sp_reset(const spec_plant_t *P, const double *n, float *s)
{
    for (int i = 0; i < P->np; i++) s[i] = (float)((double)P->y0[i] + n[i]);
    for (int j = 0; j < P->na; j++) s[P->np + j] = 0.5f;
    s[P->np + P->na] = 0.0f; s[P->np + P->na + 1] = 0.0f; s[P->np + P->na + 2] = 0.0f;
}
/* the plant model's clip (spec_plants.py): the larger of v and lo, then the smaller of that and hi; NaN -> lo; a zero
 * at a zero limit takes the limit's sign (written with compares: C's fmaxf leaves the sign of max(-0, +0) open) */
static float sp_clipf(float v, float lo, float hi)
{
    float t = (v > lo) ? v : lo;
    return (t < hi) ? t : hi;
}
static void sp_dynamics(const spec_plant_t *P, const float *s, const float *a, const double *nz, float dt, float *o)
{
    const int np = P->np, na = P->na;
    float pn[10], e = 0.0f;
    for (int j = 0; j < na; j++) {
        pn[j] = sp_clipf(fmaf(P->rate[j] * a[j], dt, s[np + j]), 0.0f, 1.0f);
        e = fmaf(P->ecost[j], pn[j], e);
    }
    for (int i = 0; i < np; i++) {
        float dy = (-P->k[i]) * (s[i] - P->amb[i]);
        for (int j = 0; j < na; j++) if (P->G[i][j] != 0.0f) dy = fmaf(P->G[i][j], pn[j], dy);
        if (P->cpl[i] != 0.0f) dy = fmaf(P->cpl[i], s[P->cidx[i]] - s[i], dy);
        if (i < 2) dy = dy + (float)nz[i];
        o[i] = sp_clipf(fmaf(dy, dt, s[i]), P->ymin[i], P->ymax[i]);
    }
    for (int j = 0; j < na; j++) o[np + j] = pn[j];
    o[np + na] = e;
    o[np + na + 1] = fmaf(e, dt, s[np + na + 1]);
    o[np + na + 2] = s[np + na + 2] + dt;
}
static float sp_reward(const spec_plant_t *P, const float *n, const float *a)
{
    float r = 0.0f, ap = 0.0f;
    for (int i = 0; i < P->np; i++) if (P->w[i] != 0.0f) r = fmaf(-P->w[i], fabsf(n[i] - P->sp[i]), r);
    r = fmaf(-P->we, n[P->np + P->na], r);
    for (int j = 0; j < P->na; j++) ap = ap + fabsf(a[j]);
    r = fmaf(-P->wu, ap, r);
    return sp_box_ok(P, 0, n) ? (r + P->bonus) : r;
}
static int sp_done(const spec_plant_t *P, const float *n) { return n[P->d_idx] < P->dlo || n[P->d_idx] > P->dhi; }

static void spec_tables_init(void)
{
    static int done_ = 0;
    if (done_) return;
    for (int k = 0; k < 4; k++) {
        const spec_plant_t *P = &SPEC_PLANTS[k];
        oracle_spec_t *sp = &SPECS[ORACLE_SPEC0 + k];
        sp->state_dim = P->np + P->na + 3; sp->action_dim = P->na; sp->n_constraints = 3;
        sp->k_step = 2; sp->k_reset = P->np; sp->max_episode_steps = SPEC_MAXSTEPS[k]; sp->dt = 0.1;
        for (int c = 0; c < 3; c++) { sp->penalty[c] = (double)P->pen[c]; sp->critical[c] = P->crit[c]; }
    }
    done_ = 1;
}
__attribute__((constructor)) static void spec_tables_ctor(void) { spec_tables_init(); }

int oracle_spec(int env, oracle_spec_t *out)
{
    if (env < 0 || env >= ORACLE_NUM_ENVS) return -1;
    *out = SPECS[env];
    return 0;
}

/* ------------------------------------------------------------------------------
 * ChemicalReactor-v0   (chemical_reactor.py)
 * ---------------------------------------------------------------------------- */
/* _get_initial_state, chemical_reactor.py:89-107: fp64 sums, stored float32 */
static void cr_reset(const double *n, float *s)
{
    s[0] = (float)(320.0 + n[0]);
    s[1] = (float)(253312.5 + n[1]);
    s[2] = (float)(50.0 + n[2]);
    s[3] = (float)(30.0 + n[3]);
    s[4] = (float)(0.5 + n[4]);
    s[5] = (float)(95.0 + n[5]);
    s[6] = (float)(295.0 + n[6]);
    s[7] = 0.0f; s[8] = 0.0f; s[9] = 0.0f;
    s[10] = (float)(60.0 + n[7]);
    s[11] = 0.0f;
}

/* _dynamics, chemical_reactor.py:109-226.  All float32 (float32 action, NumPy>=2). */
static void cr_dynamics(const float *s, const float *a, const double *noise, int flavor, float *o)
{
    float temp = s[0], pressure = s[1], cool = s[2], feed = s[3], conc = s[4], cat = s[5];
    float hx = s[6], relief = s[7], estop = s[8], alarm = s[9], level = s[10], bt = s[11];
    float hp, cadj, fadj;
    if (estop < 0.5f) {                                        /* :126-134 */
        hp = a[0] * 50000.0f; cadj = a[1] * 0.1f; fadj = a[2] * 0.1f;
    } else {
        hp = -10000.0f; cadj = 0.1f; fadj = -0.1f;
    }
    float rh = ((0.1f * conc) * (cat / 100.0f)) * 10000.0f;    /* :137-140 */
    float ch = ((cool * 100.0f) * (temp - hx)) * 0.1f;         /* :141 */
    float dT = ((hp + rh) - ch) / 418000.0f;                   /* :143-146 */
    dT = dT + (float)noise[0];                                 /* :149 */
    float nT = temp + dT * 0.1f;                               /* :151 */
    float pft = pressure * (nT / temp);                        /* :155 */
    float pfr = (conc * 0.1f) * 1000.0f;                       /* :156 */
    float nP = pft + pfr * 0.1f;                               /* :158 */
    nP = nP + (float)noise[1];                                 /* :159 */
    float nrel = pymaxf(0.0f, pyminf(100.0f, relief + (nP - 506625.0f) * 0.001f)); /* :162-163 */
    if (nrel > 0.0f) {                                         /* :166-168 */
        float pr = (nrel * 0.01f) * 10000.0f;
        nP = pymaxf(101325.0f, nP - pr);
    }
    float ncool = pymaxf(10.0f, pyminf(100.0f, cool + cadj));  /* :171 */
    float nfeed = pymaxf(5.0f, pyminf(50.0f, feed + fadj));    /* :172 */
    float rr = ((0.1f * conc) * (cat / 100.0f)) * o_expf((-(nT - 320.0f)) / 20.0f, flavor); /* :175-178 */
    float fd = nfeed * 0.001f;                                 /* :180 */
    float nconc = pymaxf(0.0f, conc + (rr - fd) * 0.1f);       /* :181-182 */
    float deact = (nT > 340.0f) ? 0.001f : 0.0001f;            /* :185 */
    float ncat = pymaxf(50.0f, cat - deact);                   /* :186 */
    float nhx = hx + (0.1f * ((290.0f + cool * 0.1f) - hx)) * 0.1f; /* :189-190 */
    float nestop = estop, nalarm = alarm;                      /* :193-194 */
    if (nT > 345.0f || nP > 480000.0f) nalarm = 1.0f;          /* :196-197 */
    if (nT > 350.0f || nP > 506625.0f) { nestop = 1.0f; nalarm = 1.0f; } /* :199-201 */
    float lc = (nfeed - 20.0f) * 0.1f;                         /* :204 */
    float nlevel = pymaxf(0.0f, pyminf(100.0f, level + lc * 0.1f)); /* :205 */
    float nbt = bt + 0.1f;                                     /* :208 */
    o[0] = nT; o[1] = nP; o[2] = ncool; o[3] = nfeed; o[4] = nconc; o[5] = ncat; o[6] = nhx;
    o[7] = nrel; o[8] = nestop; o[9] = nalarm; o[10] = nlevel; o[11] = nbt;
}

/* _compute_reward, chemical_reactor.py:228-270 (float32 accumulation) */
static float cr_reward(const float *n, const float *a)
{
    float r = 0.0f;
    r = r + n[4] * 100.0f;                                     /* :242 */
    r = r - fabsf(n[0] - 320.0f) * 0.5f;                       /* :245-246 */
    r = r - (fabsf(n[1] - 253312.5f) / 1000.0f) * 0.1f;        /* :249-250 */
    r = r + (n[5] / 100.0f) * 10.0f;                           /* :253 */
    if (30.0f <= n[10] && n[10] <= 80.0f) r = r + 5.0f;        /* :256-259 */
    else r = r - fabsf(n[10] - 55.0f) * 0.2f;
    if (n[9] > 0.5f) r = r - 50.0f;                            /* :262-263 */
    if (n[8] > 0.5f) r = r - 200.0f;                           /* :264-265 */
    float ap = ((0.0f + fabsf(a[0])) + fabsf(a[1])) + fabsf(a[2]); /* np.sum, n<8: sequential :268 */
    r = r - ap * 0.1f;                                         /* :268-269 */
    return r;
}

/* _is_done, chemical_reactor.py:272-290 */
static int cr_done(const float *s) { return s[8] > 0.5f || s[10] < 5.0f || s[10] > 95.0f || s[11] > 50.0f; }

/* constraints, chemical_reactor.py:292-305 (pre-state); 1 = satisfied */
static void cr_checks(const float *s, const float *a, int *ok)
{
    (void)a;
    ok[0] = s[0] <= 350.0f;
    ok[1] = s[1] <= 506625.0f;
    ok[2] = (20.0f <= s[10]) && (s[10] <= 90.0f);
}

/* ------------------------------------------------------------------------------
 * PowerGrid-v0   (power_grid.py)
 * ---------------------------------------------------------------------------- */
static const double PG_BASE_LOAD[8] = {50, 60, 45, 55, 40, 65, 35, 50};   /* power_grid.py:82 (int64 array) */
static const double PG_COST[8] = {25, 30, 28, 35, 32, 27, 40, 33};        /* power_grid.py:88 (int64 array) */

/* _get_initial_state, power_grid.py:90-110.  noise = [8 V normals][8 gen normals][8 load uniforms][7 flow normals] */
static void pg_reset(const double *n, float *s)
{
    s[0] = 0.0f;
    for (int i = 0; i < 8; i++) s[1 + i] = (float)(1.0 + n[i]);                       /* :98 */
    for (int i = 0; i < 8; i++) s[9 + i] = (float)(PG_BASE_LOAD[i] + n[8 + i]);       /* :101 */
    for (int i = 0; i < 8; i++) s[17 + i] = (float)(PG_BASE_LOAD[i] * (1.0 + n[16 + i])); /* :104-105 */
    for (int i = 0; i < 7; i++) s[25 + i] = (float)n[24 + i];                         /* :108 */
}

/* _dynamics, power_grid.py:112-153 */
static void pg_dynamics(const float *s, const float *a, const double *noise, double dt, float *o)
{
    float f = s[0];
    float ngen[8];
    for (int i = 0; i < 8; i++) {                              /* :124 np.clip(gen + a, 0, 100) in float32 */
        float g = s[9 + i] + a[i];
        g = (g < 0.0f) ? 0.0f : g;                             /* np.clip == minimum(maximum(x, lo), hi) */
        g = (g > 100.0f) ? 100.0f : g;
        ngen[i] = g;
    }
    float tg = sum8f(ngen);                                    /* :127 */
    float tl = sum8f(&s[17]);                                  /* :128 */
    float imb = tg - tl;                                       /* :129 */
    float fd = ((-1.0f * f) + imb) / 5.0f;                     /* :132 */
    float nf = f + fd * (float)dt;                             /* :133 */
    o[0] = nf;
    for (int i = 0; i < 8; i++) o[1 + i] = (float)((double)s[1 + i] + noise[i]);      /* :136-137 */
    for (int i = 0; i < 8; i++) o[9 + i] = ngen[i];
    for (int i = 0; i < 8; i++) {                              /* :140-141 np.maximum(loads + d, 0) fp64 */
        double l = (double)s[17 + i] + noise[8 + i];
        l = (l < 0.0) ? 0.0 : l;                               /* NaN propagates in np.maximum; l<0 false -> keeps NaN */
        o[17 + i] = (float)l;
    }
    for (int i = 0; i < 7; i++) o[25 + i] = (float)((double)s[25 + i] + noise[16 + i]); /* :144 */
}

/* _compute_reward, power_grid.py:155-177 -> Python float (fp64) */
static double pg_reward(const float *n, const float *a)
{
    float fr = -100.0f * (n[0] * n[0]);                        /* :162 */
    float dev2[8], a2[8];
    for (int i = 0; i < 8; i++) { float d = fabsf(n[1 + i] - 1.0f); dev2[i] = d * d; } /* :165-166 */
    float vr = -50.0f * sum8f(dev2);
    double cg[8];
    for (int i = 0; i < 8; i++) cg[i] = PG_COST[i] * (double)n[9 + i];                 /* :169 int64*f32 -> f64 */
    double er = (-sum8d(cg)) / 1000.0;                         /* :170 */
    for (int i = 0; i < 8; i++) a2[i] = a[i] * a[i];
    float ap = -5.0f * sum8f(a2);                              /* :173 */
    return (((double)(fr + vr)) + er) + (double)ap;            /* :175 */
}

/* _is_done, power_grid.py:179-192 (float32 compares against weak Python floats) */
static int pg_done(const float *s)
{
    if (fabsf(s[0]) > 1.0f) return 1;
    for (int i = 0; i < 8; i++) if (s[1 + i] < 0.9f || s[1 + i] > 1.1f) return 1;
    return 0;
}

/* module-level constraints, power_grid.py:10-30 */
static void pg_checks(const float *s, const float *a, int *ok)
{
    ok[0] = fabsf(s[0]) < 0.5f;
    int v = 1, g = 1;
    for (int i = 0; i < 8; i++) if (!(s[1 + i] >= 0.95f && s[1 + i] <= 1.05f)) v = 0;
    for (int i = 0; i < 8; i++) {
        float ng = s[9 + i] + a[i];                            /* float32 add; compared with 0 and f64 100 */
        if (!(ng >= 0.0f && (double)ng <= 100.0)) g = 0;
    }
    ok[1] = v; ok[2] = g;
}

/* ------------------------------------------------------------------------------
 * RobotAssembly-v0   (robot_assembly.py)
 * ---------------------------------------------------------------------------- */
static const double RA_L[7] = {0.3, 0.3, 0.25, 0.25, 0.15, 0.1, 0.05};   /* robot_assembly.py:85 */
static const double RA_TGT[3] = {0.3, 0.0, 0.4};                          /* :90 */
#define RA_PI 3.141592653589793

/* _forward_kinematics, robot_assembly.py:94-111 (fp64, sequential in joint order) */
static void ra_fk(const double *q, int flavor, double *p)
{
    double x = 0.0, y = 0.0, z = 0.0;
    for (int i = 0; i < 7; i++) {
        double sn, cs;
        o_sincos(q[i], flavor, &sn, &cs);
        if (i % 2 == 0) { x += RA_L[i] * cs; z += RA_L[i] * sn; }
        else { y += RA_L[i] * sn; }
    }
    p[0] = x; p[1] = y; p[2] = z;
}

/* _get_initial_state, robot_assembly.py:113-137.  noise = the 7 uniform joint draws themselves */
static void ra_reset(const double *n, int flavor, float *s)
{
    double p[3];
    ra_fk(n, flavor, p);
    memset(s, 0, 24 * sizeof(float));
    s[0] = (float)p[0]; s[1] = (float)p[1]; s[2] = (float)p[2];
    s[3] = 0.0f; s[4] = 0.0f; s[5] = 0.0f; s[6] = 1.0f;
    for (int i = 0; i < 7; i++) s[7 + i] = (float)n[i];
}

/* _dynamics, robot_assembly.py:139-188 */
static void ra_dynamics(const float *s, const float *a, double dt, int flavor, float *o)
{
    double q[7], p[3];
    for (int i = 0; i < 7; i++) {
        float nq = s[7 + i] + a[i] * (float)dt;                /* :148 float32 */
        double d = (double)nq;                                 /* :149-153 clip against fp64 limits */
        d = (d < -RA_PI) ? -RA_PI : d;
        d = (d > RA_PI) ? RA_PI : d;
        q[i] = d;
    }
    ra_fk(q, flavor, p);                                       /* :156 */
    double v[3];
    for (int i = 0; i < 3; i++) v[i] = (p[i] - (double)s[i]) / dt;  /* :159-160 */
    double dx = p[0] - RA_TGT[0], dy = p[1] - RA_TGT[1], dz = p[2] - RA_TGT[2];
    double dist = sqrt(dx * dx + dy * dy + dz * dz);           /* :163 np.linalg.norm */
    double F[3] = {0.0, 0.0, 0.0};
    if (dist < 0.01) {                                         /* :164-169 */
        double nf = pymaxd(0.0, 0.01 - dist) * 1000.0;
        F[2] = 0.0 - nf;                                       /* -0 (int) when nf == 0 -> +0.0 stored */
        if (nf == 0.0) F[2] = 0.0;
    }
    double ae = sqrt(dx * dx + dy * dy);                       /* :172 */
    double align = pymaxd(0.0, 1.0 - ae / 0.005);              /* :173 */
    double ins = pymaxd(0.0, RA_TGT[2] - p[2]);                /* :175 */
    double depth = pymind(1.0, ins / 0.05);                    /* :176 */
    double compl = align * depth;                              /* :178 */
    memcpy(o, s, 24 * sizeof(float));
    o[0] = (float)p[0]; o[1] = (float)p[1]; o[2] = (float)p[2];
    o[3] = 0.0f; o[4] = 0.0f; o[5] = 0.0f; o[6] = 1.0f;        /* :182 */
    for (int i = 0; i < 7; i++) o[7 + i] = (float)q[i];        /* :183 */
    o[14] = (float)v[0]; o[15] = (float)v[1]; o[16] = (float)v[2]; o[17] = 0.0f; /* :184 */
    o[18] = (float)F[0]; o[19] = (float)F[1]; o[20] = (float)F[2];
    o[21] = (float)align; o[22] = (float)depth; o[23] = (float)compl;
}

/* _compute_reward, robot_assembly.py:190-222 -> Python float */
static double ra_reward(const float *n, const float *a)
{
    float cr = 100.0f * n[23];                                 /* :197 */
    double dx = (double)n[0] - RA_TGT[0], dy = (double)n[1] - RA_TGT[1], dz = (double)n[2] - RA_TGT[2];
    double dr = -10.0 * sqrt(dx * dx + dy * dy + dz * dz);     /* :200-201 */
    float fm = sqrtf(n[18] * n[18] + n[19] * n[19] + n[20] * n[20]);  /* :204 float32 norm */
    float ap = 0.0f, vp = 0.0f;
    for (int i = 0; i < 7; i++) ap = ap + a[i] * a[i];         /* :211 sequential (n<8) */
    ap = -0.1f * ap;
    for (int i = 0; i < 4; i++) vp = vp + n[14 + i] * n[14 + i]; /* :215 */
    vp = -0.5f * vp;
    double tot = (double)cr + dr;                              /* :217-220 left-to-right */
    if (fm > 30.0f) tot = tot + (double)(-50.0f * (fm - 30.0f)); else tot = tot + 0.0;
    tot = tot + (double)ap;
    tot = tot + (double)vp;
    return tot;
}

/* _is_done, robot_assembly.py:224-244 */
static int ra_done(const float *s)
{
    if (s[23] > 0.95f) return 1;
    for (int i = 0; i < 3; i++) if (fabsf(s[18 + i]) > 80.0f) return 1;
    static const double lo[3] = {-0.6, -0.6, -0.1}, hi[3] = {0.6, 0.6, 0.9};
    for (int i = 0; i < 3; i++) if (!((double)s[i] >= lo[i] && (double)s[i] <= hi[i])) return 1;
    return 0;
}

/* module-level constraints, robot_assembly.py:10-32 */
static void ra_checks(const float *s, const float *a, int *ok)
{
    (void)a;
    int f = 1, c = 1, v = 1;
    for (int i = 0; i < 3; i++) if (!(fabsf(s[18 + i]) < 50.0f)) f = 0;
    static const double lo[3] = {-0.5, -0.5, 0.0}, hi[3] = {0.5, 0.5, 0.8};
    for (int i = 0; i < 3; i++) if (!((double)s[i] >= lo[i] && (double)s[i] <= hi[i])) c = 0;
    for (int i = 0; i < 7; i++) if (!(fabsf(s[7 + i]) < 2.0f)) v = 0;
    ok[0] = f; ok[1] = c; ok[2] = v;
}


/* ------------------------------------------------------------------------------
 * AdvancedChemicalReactor-v0 / AdvancedPowerGrid-v0 -- CANDIDATE ROWS, PARITY UNPINNED.
 * Neither class can be instantiated upstream (abstract hooks missing; SafetyConstraint /
 * SafetyMetrics are given kwargs that do not exist: advanced_chemical_reactor.py:90-105,
 * 445-450; advanced_power_grid.py:101-121,532-537) and step() reads self.episode_step, which
 * nothing sets (:351,364 / :331,345), so there is no reference output.  Restated from the
 * source text as the float32 evaluation JAX performs with weak Python scalars and x64 off:
 * Python-only sub-expressions are folded in double first, everything touching an array value
 * is float32, left to right.  episode_step := 0 at reset.  step() is overridden wholesale:
 * no action clip, no base constraint loop, no -1000 shutdown.
 * ---------------------------------------------------------------------------- */
typedef struct {
    float reward; int terminated, truncated, viol_mask, shutdown;
} adv_out_t;

static void acr_reset(float *s)                                       /* advanced_chemical_reactor.py:158-193 */
{
    static const float init[20] = {323.15f, 313.15f, 2e5f, 2.0f, 1.5f, 0.1f, 0.1f, 0.001f, 0.001f, 0.005f, 300.0f, 0.8f,
                                   323.15f, 323.15f, 323.15f, 323.15f, 1000.0f, 0.05f, 50.0f, 60.0f};
    memcpy(s, init, sizeof init);
}

static void acr_step(const float *s, const float *a, int step_pre, int max_steps, float dt, int flavor, float *o, adv_out_t *out)
{
    float T = s[0], Tj = s[1], cA = s[3], cB = s[4], cC = s[5], cD = s[6], Ff = s[7], Fp = s[8], Fc = s[9], hc = s[10], mix = s[11];
    int estop = a[5] > 0.5f;                                           /* :219-223 */
    float feed_a = estop ? 0.0f : a[0], cool_a = estop ? 0.01f : a[1], rpm = estop ? 0.0f : a[2];
    float nFf = Ff + 0.1f * (feed_a - Ff);                             /* :226 */
    float nFc = Fc + 0.2f * (cool_a - Fc);                             /* :227 */
    float k = 1e8f * o_expf(-83140.0f / (8.314f * T), flavor);         /* :230 */
    float rr = ((k * cA) * cB) * mix;                                  /* :231 */
    float dA = ((nFf * 5.0f - Fp * cA) / 1.0f) - rr;                   /* :234-237 */
    float dB = ((nFf * 3.0f - Fp * cB) / 1.0f) - rr;
    float dC = (((-Fp) * cC) / 1.0f) + rr;
    float dD = (((-Fp) * cD) / 1.0f) + rr;
    float Qgen = (50000.0f * rr) * 1.0f;                               /* :240 */
    float Qj = (hc * 4.835975862049409f) * (T - Tj);                   /* :243, jacket_area :78 */
    float Qw = 0.0f;
    for (int i = 0; i < 4; i++) Qw = Qw + 6044.969827561761f * (T - s[12 + i]);   /* :246-250 */
    float Qf = ((nFf * 1000.0f) * 4180.0f) * (a[3] - T);               /* :253 */
    float dTr = (((Qgen - Qj) - Qw) + Qf) / 4180000.0f;                /* :256-259 */
    float dTj = (Qj - ((nFc * 1000.0f) * 4180.0f) * (Tj - 293.15f)) / 418000.0f;  /* :262-266 */
    float nTw[4];
    for (int i = 0; i < 4; i++) {                                      /* :269-280 */
        float w = s[12 + i];
        float wd = (5000.0f * (T - w) - 10.0f * (w - 293.15f)) / 25000.0f;
        nTw[i] = w + dt * wd;
    }
    float moles = (((cA + cB) + cC) + cD) * 1.0f;                      /* :284 */
    float vp = 1000.0f * o_expf(20.0f - 5000.0f / T, flavor);          /* :287 */
    float nP = ((((8.314f * T) * moles) / 1.0f) + vp) + 1e5f;          /* :290-292 */
    if (nP > 2400000.0f) nP = nP - (a[4] / 100.0f) * (nP - 2400000.0f);/* :295-297 */
    float nmix = o_tanhf(rpm / 1000.0f, flavor) * 0.9f + 0.1f;         /* :300 */
    float Re = ((rpm * 0.1f) * 1000.0f) / 0.001f;                      /* :301 */
    float Nu = 0.023f * o_powf(Re, 0.8f, flavor);                      /* :302 */
    float nhc = (Nu * 0.6f) / 0.1f;                                    /* :303 */
    float nFp = 0.001f * (1.0f + 0.5f * ((nP - 1e5f) / 1e5f));         /* :306-307 */
    float nA = fmaxf(0.0f, cA + dt * dA), nB = fmaxf(0.0f, cB + dt * dB), nC = fmaxf(0.0f, cC + dt * dC), nD = fmaxf(0.0f, cD + dt * dD);
    float nT = T + dt * dTr, nTj = Tj + dt * dTj;                      /* :315-316 */
    float tau = 1.0f / fmaxf(nFp, 1e-6f);                              /* :319 */
    float conv = (2.0f - nA) / 2.0f;                                   /* :322-323 */
    float mT = ((673.15f - nT) / 673.15f) * 100.0f, mP = ((5e6f - nP) / 5e6f) * 100.0f;   /* :326-327 */
    float st[20] = {nT, nTj, nP, nA, nB, nC, nD, nFf, nFp, nFc, nhc, nmix, nTw[0], nTw[1], nTw[2], nTw[3], tau, conv, mT, mP};
    memcpy(o, st, sizeof st);
    float pr = 100.0f * (nC / 5.0f + conv);                            /* :379 */
    float sr = (mT + mP) / 2.0f;                                       /* :382 */
    float te = 1.0f - fabsf(nT - 373.15f) / 100.0f, pe = 1.0f - fabsf(nP - 3e5f) / 1e5f;  /* :385-386 */
    float er = 50.0f * (te + pe);                                      /* :388 */
    float cp = (-((((fabsf(a[0]) + fabsf(a[1])) + fabsf(a[2])) + fabsf(a[3])) + fabsf(a[4]))) * 10.0f;   /* :391 */
    float ep = estop ? -1000.0f : 0.0f;                                /* :394 */
    out->reward = (((pr + sr) + er) + cp) + ep;                        /* :396-402 */
    out->viol_mask = ((nT > 673.15f) ? 1 : 0) | ((nP > 5e6f) ? 2 : 0) | ((mT < 10.0f) ? 4 : 0) | ((mP < 10.0f) ? 8 : 0);  /* :433-443 */
    out->terminated = (nT > 673.15f) || (nP > 5e6f) || (nC > 8.0f);    /* :412-420 */
    out->truncated = step_pre >= max_steps;                            /* :351 */
    out->shutdown = estop;                                             /* :359 */
}

static void apg_reset(float *s)                                        /* advanced_power_grid.py:182-226 */
{
    static const float init[32] = {1, 1, 1, 1, 1, 1, 1, 1, 0.0f, -0.1f, 0.05f, -0.05f, 0.02f, -0.02f, 0.08f, -0.08f,
                                   50, 50, 50, 50, 30, 25, 20, 28, 25, 20, 30, 18, 15, -12, 18, -14};
    memcpy(s, init, sizeof init);
}

static void apg_step(const float *s, const float *a, int step_pre, int max_steps, float dt, int flavor, float *o, adv_out_t *out)
{
    static const float H[4] = {5.0f, 4.0f, 3.5f, 4.5f}, D[4] = {1.0f, 0.8f, 0.9f, 1.1f};          /* :79-85 */
    static const float Pmax[4] = {50.0f, 40.0f, 35.0f, 45.0f}, Pmin[4] = {10.0f, 8.0f, 7.0f, 9.0f}, ramp[4] = {2.0f, 1.8f, 1.5f, 2.2f};
    static const float bl0[4] = {25.0f, 20.0f, 30.0f, 18.0f}, al[4] = {1.5f, 1.2f, 1.8f, 1.3f}, Kf[4] = {1.0f, 0.8f, 1.2f, 0.9f};  /* :93-97 */
    int emerg = a[7] > 0.5f;                                           /* :246-249 */
    float shed = emerg ? fminf(a[6] + 10.0f, 30.0f) : a[6];
    float sp[4], nf[4], nPg[4], nL[4], fsum = 0.0f;
    for (int i = 0; i < 4; i++) {
        sp[i] = emerg ? a[i] * 0.7f : a[i];
        float pm = sp[i] / 100.0f, pe = s[20 + i] / 100.0f;            /* :261-262 */
        float df = ((pm - pe) - D[i] * (s[16 + i] - 50.0f)) / (2.0f * H[i]);   /* :264-265 */
        nf[i] = s[16 + i] + dt * df;                                   /* :272 */
        fsum = fsum + nf[i] * H[i];                                    /* :276 */
    }
    float fsys = fsum / 17.0f;
    for (int i = 0; i < 4; i++) {                                      /* :279-289 */
        float mr = ramp[i] * dt, ch = sp[i] - s[20 + i];
        ch = fminf(fmaxf(ch, -mr), mr);
        nPg[i] = fminf(fmaxf(s[20 + i] + ch, Pmin[i]), Pmax[i]);
    }
    float fdev = (fsys - 50.0f) / 50.0f;                               /* :304 */
    for (int i = 0; i < 4; i++) {                                      /* :293-308 */
        float bl = bl0[i];
        if (i == 0) bl = fmaxf(bl - shed, 0.0f);
        float ve = o_powf(s[i] / 1.0f, al[i], flavor);
        float fe = 1.0f + Kf[i] * fdev;
        nL[i] = (bl * ve) * fe;
    }
    float nV[8], nTh[8];
    for (int i = 0; i < 8; i++) {                                      /* :368-389 */
        float inj = (i < 4) ? nPg[i] / 100.0f : (-nL[i - 4]) / 100.0f;
        float v = s[i] + 0.01f * inj;
        if (i == 0) v = a[4];
        if (i == 1) v = a[5];
        nV[i] = fminf(fmaxf(v, 0.8f), 1.2f);
        nTh[i] = s[8 + i] + 0.05f * inj;
    }
    float flow[4];
    for (int i = 0; i < 4; i++) flow[i] = (((nV[i] * nV[i + 4]) / 0.1f) * o_sinf(nTh[i] - nTh[i + 4], flavor)) * 100.0f;   /* :395-405 */
    float vmax = 0.0f, vmean = 0.0f, thmax = nTh[0], thmin = nTh[0], fmaxd = 0.0f;
    int vviol = 0;
    for (int i = 0; i < 8; i++) {
        float dv = fabsf(nV[i] - 1.0f);
        vmax = fmaxf(vmax, dv); vmean = vmean + dv;
        if (dv > 0.05f) vviol = 1;
        thmax = fmaxf(thmax, nTh[i]); thmin = fminf(thmin, nTh[i]);
    }
    vmean = vmean / 8.0f;
    for (int i = 0; i < 4; i++) fmaxd = fmaxf(fmaxd, fabsf(nf[i] - 50.0f));
    float stab = fmaxf(fminf(fminf(1.0f - vmax, 1.0f - (thmax - thmin) / 3.14159265358979323846f), 1.0f - fmaxd / 0.5f), 0.0f);   /* :417-434 */
    for (int i = 0; i < 8; i++) { o[i] = nV[i]; o[8 + i] = nTh[i]; }
    for (int i = 0; i < 4; i++) { o[16 + i] = nf[i]; o[20 + i] = nPg[i]; o[24 + i] = nL[i]; o[28 + i] = flow[i]; }
    float ferr = fabsf(fsys - 50.0f);                                  /* :446-480 */
    float r_f = 100.0f * o_expf((-ferr) / 0.1f, flavor);
    float r_v = 50.0f * o_expf((-vmean) / 0.05f, flavor);
    float tg = ((nPg[0] + nPg[1]) + nPg[2]) + nPg[3], tl = ((nL[0] + nL[1]) + nL[2]) + nL[3];
    float r_b = 30.0f * o_expf((-fabsf(tg - tl)) / 10.0f, flavor);
    float r_e = -(0.01f * ((((nPg[0] * nPg[0]) + (nPg[1] * nPg[1])) + (nPg[2] * nPg[2])) + (nPg[3] * nPg[3])));
    float r_c = (-(((((fabsf(a[0]) + fabsf(a[1])) + fabsf(a[2])) + fabsf(a[3])) + fabsf(a[4])) + fabsf(a[5]))) * 1.0f;
    out->reward = (((((r_f + r_v) + r_b) + r_e) + r_c) + (-a[6]) * 50.0f) + (-a[7]) * 200.0f;
    int glim = 0;
    for (int i = 0; i < 4; i++) if (nPg[i] < Pmin[i] || nPg[i] > Pmax[i]) glim = 1;   /* :521-523 */
    out->viol_mask = ((ferr > 0.5f) ? 1 : 0) | (vviol ? 2 : 0) | (glim ? 4 : 0);
    out->terminated = (ferr > 0.5f) || vviol || (stab < 0.1f);         /* :492-501 */
    out->truncated = step_pre >= max_steps;                            /* :331 */
    out->shutdown = emerg;
}

static const float ACT_LOW_[5][8] = {{-1, -1, -1}, {-1, -1, -1, -1, -1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1, -1},
                                    {0, 0, 0, 273.15f, 0, 0}, {10, 8, 7, 9, 0.95f, 0.95f, 0, 0}};
static const float ACT_HIGH_[5][8] = {{1, 1, 1}, {1, 1, 1, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1, 1},
                                     {0.01f, 0.01f, 3000, 473.15f, 100, 1}, {50, 40, 35, 45, 1.05f, 1.05f, 20, 1}};

static float act_low(int env, int i) { return env < 5 ? ACT_LOW_[env][i] : -1.0f; }
static float act_high(int env, int i) { return env < 5 ? ACT_HIGH_[env][i] : 1.0f; }

/* ------------------------------------------------------------------------------
 * IndustrialEnv.reset / IndustrialEnv.step   (base.py:133-213)
 * ---------------------------------------------------------------------------- */
void oracle_reset(int env, const double *noise, int flavor, float *state)
{
    if (env == ORACLE_CR) cr_reset(noise, state);
    else if (env == ORACLE_PG) pg_reset(noise, state);
    else if (env == ORACLE_RA) ra_reset(noise, flavor, state);
    else if (env == ORACLE_ACR) acr_reset(state);
    else if (env == ORACLE_APG) apg_reset(state);
    else sp_reset(&SPEC_PLANTS[env - ORACLE_SPEC0], noise, state);
}

typedef struct {
    double reward;        /* CR: exactly a float32 value; PG/RA: fp64 Python float */
    int terminated, truncated;
    int violation_count, critical_violations;   /* SafetyMetrics of this step (base.py:94-124) */
    int ok[3];            /* per-constraint: 1 satisfied */
    int viol_mask;        /* bit k: condition k violated (the Advanced envs have up to 4) */
    int shutdown;         /* info['critical_shutdown'] / info['emergency_shutdown'|'emergency_active'] */
} oracle_step_out_t;

/* One IndustrialEnv.step on one env instance.  step_pre = current_step before the call. */
void oracle_step(int env, const float *state, const float *action_raw, const double *noise,
                 int step_pre, int max_steps, double dt, int flavor,
                 float *next, oracle_step_out_t *out)
{
    const oracle_spec_t *sp = &SPECS[env];
    if (env == ORACLE_ACR || env == ORACLE_APG) {              /* step() overridden wholesale */
        adv_out_t ao;
        if (env == ORACLE_ACR) acr_step(state, action_raw, step_pre, max_steps, (float)dt, flavor, next, &ao);
        else apg_step(state, action_raw, step_pre, max_steps, (float)dt, flavor, next, &ao);
        out->reward = (double)ao.reward; out->terminated = ao.terminated; out->truncated = ao.truncated;
        out->viol_mask = ao.viol_mask; out->violation_count = __builtin_popcount(ao.viol_mask);
        out->critical_violations = 0; out->shutdown = ao.shutdown;
        for (int k = 0; k < 3; k++) out->ok[k] = !((ao.viol_mask >> k) & 1);
        return;
    }
    float a[10];
    for (int i = 0; i < sp->action_dim; i++) {                 /* base.py:167 np.clip(action, -1, 1) */
        float x = action_raw[i];
        x = (x < -1.0f) ? -1.0f : x;
        x = (x > 1.0f) ? 1.0f : x;
        a[i] = x;
    }
    int ok[3];
    const spec_plant_t *SP = env >= ORACLE_SPEC0 ? &SPEC_PLANTS[env - ORACLE_SPEC0] : NULL;
    if (env == ORACLE_CR) cr_checks(state, a, ok);             /* base.py:170 */
    else if (env == ORACLE_PG) pg_checks(state, a, ok);
    else if (env == ORACLE_RA) ra_checks(state, a, ok);
    else for (int c = 0; c < 3; c++) ok[c] = sp_box_ok(SP, c, state);
    int viol = 0, crit = 0;
    for (int k = 0; k < 3; k++) if (!ok[k]) { viol++; if (sp->critical[k]) crit++; }

    double reward;
    if (env == ORACLE_CR || SP) {                              /* base.py:173-183 */
        float r;
        if (SP) { sp_dynamics(SP, state, a, noise, (float)dt, next); r = sp_reward(SP, next, a); }
        else { cr_dynamics(state, a, noise, flavor, next); r = cr_reward(next, a); }
        for (int k = 0; k < 3; k++) if (!ok[k]) r = r + (float)sp->penalty[k];
        if (crit > 0) r = r - 1000.0f;                         /* base.py:195-198 */
        reward = (double)r;
    } else {
        double r;
        if (env == ORACLE_PG) { pg_dynamics(state, a, noise, dt, next); r = pg_reward(next, a); }
        else { ra_dynamics(state, a, dt, flavor, next); r = ra_reward(next, a); }
        for (int k = 0; k < 3; k++) if (!ok[k]) r = r + sp->penalty[k];
        if (crit > 0) r = r - 1000.0;
        reward = r;
    }
    int step = step_pre + 1;                                   /* base.py:187 */
    int term = SP ? sp_done(SP, next) : (env == ORACLE_CR) ? cr_done(next) : (env == ORACLE_PG) ? pg_done(next) : ra_done(next);
    int trunc = step >= max_steps;                             /* base.py:191 */
    if (crit > 0) term = 1;                                    /* base.py:195-197 */
    out->reward = reward;
    out->terminated = term; out->truncated = trunc;
    out->violation_count = viol; out->critical_violations = crit;
    for (int k = 0; k < 3; k++) out->ok[k] = ok[k];
    out->viol_mask = (!ok[0] ? 1 : 0) | (!ok[1] ? 2 : 0) | (!ok[2] ? 4 : 0);
    out->shutdown = crit > 0;
}

/* ------------------------------------------------------------------------------
 * FLOAT64 ACTIONS.  The reference's own callers hand np.float64 arrays to step() (get_dataset:
 * chemical_reactor.py:364-393, power_grid.py:216-233, robot_assembly.py:266-290; baseline agents:
 * benchmarks/baseline_agents.py:28-114), and base.py:167 clips without casting (np.clip of a float64
 * array against float32 bounds stays float64).  Under NumPy >= 2 every expression that touches an
 * action element is then float64, and float64 spreads through what depends on it until a value is
 * stored into the float32 state vector.  Restated per env below; pinned by tests/golden/<env>_g5.npz
 * (float32-valued float64 actions) and <env>_g6.npz (genuine float64 action values).
 * ---------------------------------------------------------------------------- */
static double det_exp64(double x);      /* fdlibm-style e^x (MATH_POLY), below */
static double o_exp64(double x, int flavor) { return flavor == MATH_POLY ? det_exp64(x) : exp(x); }

/* chemical_reactor.py:109-226 with a float64 action vector */
static void cr_dynamics64(const float *s, const double *a, const double *noise, int flavor, float *o)
{
    float temp = s[0], pressure = s[1], cool = s[2], feed = s[3], conc = s[4], cat = s[5];
    float hx = s[6], relief = s[7], estop = s[8], alarm = s[9], level = s[10], bt = s[11];
    if (!(estop < 0.5f)) {              /* emergency branch :131-134: the action is not read, everything stays float32 */
        const float zero[3] = {0.0f, 0.0f, 0.0f};
        cr_dynamics(s, zero, noise, flavor, o);
        return;
    }
    double hp = a[0] * 50000.0, cadj = a[1] * 0.1, fadj = a[2] * 0.1;           /* :127-129 float64 */
    float kc = (0.1f * conc) * (cat / 100.0f);                                   /* :137-139 float32 */
    float rh = kc * 10000.0f;
    float ch = ((cool * 100.0f) * (temp - hx)) * 0.1f;                           /* :141 float32 */
    double dT = ((hp + (double)rh) - (double)ch) / 418000.0;                     /* :143-146 */
    dT = dT + noise[0];                                                          /* :149 */
    double nT = (double)temp + dT * 0.1;                                         /* :151 */
    double pft = (double)pressure * (nT / (double)temp);                         /* :155 */
    float pfr = (conc * 0.1f) * 1000.0f;                                         /* :156 float32 */
    double nP = pft + (double)(pfr * 0.1f);                                      /* :158 */
    nP = nP + noise[1];                                                          /* :159 */
    double nrel = pymaxd(0.0, pymind(100.0, (double)relief + (nP - 506625.0) * 0.001));   /* :162-163 */
    if (nrel > 0.0) nP = pymaxd(101325.0, nP - (nrel * 0.01) * 10000.0);         /* :166-168 */
    double ncool = pymaxd(10.0, pymind(100.0, (double)cool + cadj));             /* :171 */
    double nfeed = pymaxd(5.0, pymind(50.0, (double)feed + fadj));               /* :172 */
    double rr = (double)kc * o_exp64((-(nT - 320.0)) / 20.0, flavor);            /* :175-178 np.exp on a float64 scalar */
    double fd = nfeed * 0.001;                                                   /* :180 */
    double nconc = pymaxd(0.0, (double)conc + (rr - fd) * 0.1);                  /* :181-182 */
    float deact = (nT > 340.0) ? 0.001f : 0.0001f;                               /* :185 */
    float ncat = pymaxf(50.0f, cat - deact);                                     /* :186 float32 */
    float nhx = hx + (0.1f * ((290.0f + cool * 0.1f) - hx)) * 0.1f;              /* :189-190 float32 (old cooling flow) */
    float nestop = estop, nalarm = alarm;
    if (nT > 345.0 || nP > 480000.0) nalarm = 1.0f;                              /* :196-197 */
    if (nT > 350.0 || nP > 506625.0) { nestop = 1.0f; nalarm = 1.0f; }           /* :199-201 */
    double lc = (nfeed - 20.0) * 0.1;                                            /* :204 */
    double nlevel = pymaxd(0.0, pymind(100.0, (double)level + lc * 0.1));        /* :205 */
    o[0] = (float)nT; o[1] = (float)nP; o[2] = (float)ncool; o[3] = (float)nfeed; o[4] = (float)nconc;
    o[5] = ncat; o[6] = nhx; o[7] = (float)nrel; o[8] = nestop; o[9] = nalarm; o[10] = (float)nlevel;
    o[11] = bt + 0.1f;                                                           /* :208-224 np.array(..., dtype=float32) */
}

/* chemical_reactor.py:228-270: float32 until the action penalty, float64 from there */
static double cr_reward64(const float *n, const double *a)
{
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    float r = cr_reward(n, zero);                              /* ... - 0.0f * 0.1f leaves r as it was */
    double ap = ((0.0 + fabs(a[0])) + fabs(a[1])) + fabs(a[2]);
    return (double)r - ap * 0.1;                               /* :268-269 */
}

/* power_grid.py:24-30 with a float64 action */
static void pg_checks64(const float *s, const double *a, int *ok)
{
    const float zero[8] = {0};
    pg_checks(s, zero, ok);
    int g = 1;
    for (int i = 0; i < 8; i++) {
        double ng = (double)s[9 + i] + a[i];
        if (!(ng >= 0.0 && ng <= 100.0)) g = 0;
    }
    ok[2] = g;
}

/* power_grid.py:112-153 with a float64 action */
static void pg_dynamics64(const float *s, const double *a, const double *noise, double dt, float *o)
{
    const float zero[8] = {0};
    pg_dynamics(s, zero, noise, dt, o);                        /* voltages, loads, line flows do not see the action */
    double ngen[8];
    for (int i = 0; i < 8; i++) {                              /* :124 np.clip(gen + a, 0, 100) in float64 */
        double g = (double)s[9 + i] + a[i];
        g = (g < 0.0) ? 0.0 : g;
        g = (g > 100.0) ? 100.0 : g;
        ngen[i] = g;
    }
    double tg = sum8d(ngen);                                   /* :127 */
    float tl = sum8f(&s[17]);                                  /* :128 float32 */
    double imb = tg - (double)tl;                              /* :129 */
    double fd = ((double)(-1.0f * s[0]) + imb) / 5.0;          /* :132  (-D * f) is float32, the sum float64 */
    double nf = (double)s[0] + fd * dt;                        /* :133 */
    o[0] = (float)nf;
    for (int i = 0; i < 8; i++) o[9 + i] = (float)ngen[i];
}

/* power_grid.py:155-177 with a float64 action */
static double pg_reward64(const float *n, const double *a)
{
    const float zero[8] = {0};
    double base = pg_reward(n, zero);                          /* ((fr + vr) + er) + (-5.0f * 0) : adding -0.0 changes nothing */
    double a2[8];
    for (int i = 0; i < 8; i++) a2[i] = a[i] * a[i];
    double ap = -5.0 * sum8d(a2);                              /* :173 */
    return base + ap;                                          /* :175 */
}

/* robot_assembly.py:139-188 with a float64 action */
static void ra_dynamics64(const float *s, const double *a, double dt, int flavor, float *o)
{
    /* the float32 form with q = joint + a*dt taken in float64 (:148): rebuild through a scratch state whose
       joints already are the float64 sums is not possible in float32, so the body is restated */
    double q[7], p[3];
    for (int i = 0; i < 7; i++) {
        double d = (double)s[7 + i] + a[i] * dt;               /* :148 float64 */
        d = (d < -RA_PI) ? -RA_PI : d;
        d = (d > RA_PI) ? RA_PI : d;
        q[i] = d;
    }
    ra_fk(q, flavor, p);
    double v[3];
    for (int i = 0; i < 3; i++) v[i] = (p[i] - (double)s[i]) / dt;
    double dx = p[0] - RA_TGT[0], dy = p[1] - RA_TGT[1], dz = p[2] - RA_TGT[2];
    double dist = sqrt(dx * dx + dy * dy + dz * dz);
    double F[3] = {0.0, 0.0, 0.0};
    if (dist < 0.01) {
        double nf = pymaxd(0.0, 0.01 - dist) * 1000.0;
        F[2] = 0.0 - nf;
        if (nf == 0.0) F[2] = 0.0;
    }
    double ae = sqrt(dx * dx + dy * dy);
    double align = pymaxd(0.0, 1.0 - ae / 0.005);
    double ins = pymaxd(0.0, RA_TGT[2] - p[2]);
    double depth = pymind(1.0, ins / 0.05);
    double compl = align * depth;
    memcpy(o, s, 24 * sizeof(float));
    o[0] = (float)p[0]; o[1] = (float)p[1]; o[2] = (float)p[2];
    o[3] = 0.0f; o[4] = 0.0f; o[5] = 0.0f; o[6] = 1.0f;
    for (int i = 0; i < 7; i++) o[7 + i] = (float)q[i];
    o[14] = (float)v[0]; o[15] = (float)v[1]; o[16] = (float)v[2]; o[17] = 0.0f;
    o[18] = (float)F[0]; o[19] = (float)F[1]; o[20] = (float)F[2];
    o[21] = (float)align; o[22] = (float)depth; o[23] = (float)compl;
}

/* robot_assembly.py:190-222 with a float64 action */
static double ra_reward64(const float *n, const double *a)
{
    float cr = 100.0f * n[23];
    double dx = (double)n[0] - RA_TGT[0], dy = (double)n[1] - RA_TGT[1], dz = (double)n[2] - RA_TGT[2];
    double dr = -10.0 * sqrt(dx * dx + dy * dy + dz * dz);
    float fm = sqrtf(n[18] * n[18] + n[19] * n[19] + n[20] * n[20]);
    double ap = 0.0;
    float vp = 0.0f;
    for (int i = 0; i < 7; i++) ap = ap + a[i] * a[i];         /* :211 float64, sequential (n < 8) */
    ap = -0.1 * ap;
    for (int i = 0; i < 4; i++) vp = vp + n[14 + i] * n[14 + i];
    vp = -0.5f * vp;
    double tot = (double)cr + dr;
    if (fm > 30.0f) tot = tot + (double)(-50.0f * (fm - 30.0f)); else tot = tot + 0.0;
    tot = tot + ap;
    tot = tot + (double)vp;
    return tot;
}

/* IndustrialEnv.step with a float64 action vector.  Envs other than the three NumPy ones convert the action to
 * float32 themselves (the Advanced envs are JAX with x64 off; the build-specified plants are float32 by design). */
void oracle_step64(int env, const float *state, const double *action_raw, const double *noise,
                   int step_pre, int max_steps, double dt, int flavor, float *next, oracle_step_out_t *out)
{
    const oracle_spec_t *sp = &SPECS[env];
    if (env != ORACLE_CR && env != ORACLE_PG && env != ORACLE_RA) {
        float a32[10];
        for (int i = 0; i < sp->action_dim; i++) a32[i] = (float)action_raw[i];
        oracle_step(env, state, a32, noise, step_pre, max_steps, dt, flavor, next, out);
        return;
    }
    double a[10];
    for (int i = 0; i < sp->action_dim; i++) {                 /* base.py:167: float64 array, float32 bounds -1, 1 */
        double x = action_raw[i];
        x = (x < -1.0) ? -1.0 : x;
        x = (x > 1.0) ? 1.0 : x;
        a[i] = x;
    }
    int ok[3];
    const float zero[10] = {0};
    if (env == ORACLE_CR) cr_checks(state, zero, ok);
    else if (env == ORACLE_PG) pg_checks64(state, a, ok);
    else ra_checks(state, zero, ok);
    int viol = 0, crit = 0;
    for (int k = 0; k < 3; k++) if (!ok[k]) { viol++; if (sp->critical[k]) crit++; }
    double r;
    if (env == ORACLE_CR) { cr_dynamics64(state, a, noise, flavor, next); r = cr_reward64(next, a); }
    else if (env == ORACLE_PG) { pg_dynamics64(state, a, noise, dt, next); r = pg_reward64(next, a); }
    else { ra_dynamics64(state, a, dt, flavor, next); r = ra_reward64(next, a); }
    for (int k = 0; k < 3; k++) if (!ok[k]) r = r + sp->penalty[k];      /* base.py:179-183 (float64 reward) */
    if (crit > 0) r = r - 1000.0;
    int step = step_pre + 1;
    int term = (env == ORACLE_CR) ? cr_done(next) : (env == ORACLE_PG) ? pg_done(next) : ra_done(next);
    int trunc = step >= max_steps;
    if (crit > 0) term = 1;
    out->reward = r; out->terminated = term; out->truncated = trunc;
    out->violation_count = viol; out->critical_violations = crit;
    for (int k = 0; k < 3; k++) out->ok[k] = ok[k];
    out->viol_mask = (!ok[0] ? 1 : 0) | (!ok[1] ? 2 : 0) | (!ok[2] ? 4 : 0);
    out->shutdown = crit > 0;
}

void oracle_step_batch64(int env, int n, const float *states, const double *actions, const double *noise,
                         const int *step_pre, int max_steps, double dt, int flavor,
                         float *next, double *reward, int *term, int *trunc, int *viol, int *crit, int *ok, int *mask)
{
    const oracle_spec_t *sp = &SPECS[env];
    for (int i = 0; i < n; i++) {
        oracle_step_out_t o;
        oracle_step64(env, states + (size_t)i * sp->state_dim, actions + (size_t)i * sp->action_dim,
                      noise ? noise + (size_t)i * sp->k_step : NULL, step_pre[i], max_steps, dt, flavor,
                      next + (size_t)i * sp->state_dim, &o);
        reward[i] = o.reward; term[i] = o.terminated; trunc[i] = o.truncated;
        viol[i] = o.violation_count; crit[i] = o.critical_violations;
        for (int k = 0; k < 3; k++) ok[i * 3 + k] = o.ok[k];
        if (mask) mask[i] = o.viol_mask | (o.shutdown << 8);
    }
}

/* e^x in double: Cody-Waite by ln2 (hi/lo), fdlibm's degree-5 kernel on r^2, exact scaling.  Stands in for
 * np.exp on a float64 scalar (chemical_reactor.py:177 with a float64 action); < 1 ulp. */
static double det_exp64(double x)
{
    if (x != x) return x;
    if (x > 709.78) return INFINITY;
    if (x < -745.13) return 0.0;
    const double k = floor(x * 1.44269504088896338700e+00 + 0.5);
    const double hi = fma(-k, 6.93147180369123816490e-01, x);
    const double lo = k * 1.90821492927058770002e-10;
    const double r = hi - lo;
    const double t = r * r;
    double c = 4.13813679705723846039e-08;
    c = fma(c, t, -1.65339022054652515390e-06);
    c = fma(c, t, 6.61375632143793436117e-05);
    c = fma(c, t, -2.77777777770155933842e-03);
    c = fma(c, t, 1.66666666666666019037e-01);
    c = r - t * c;
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    int ki = (int)k;
    const int k1 = ki / 2, k2 = ki - k1;                      /* two exact power-of-two scalings */
    union { uint64_t u; double d; } s1, s2;
    s1.u = (uint64_t)(k1 + 1023) << 52; s2.u = (uint64_t)(k2 + 1023) << 52;
    return (y * s1.d) * s2.d;
}

/* batched convenience for tests: row-major [n][S] states etc. */
void oracle_step_batch(int env, int n, const float *states, const float *actions, const double *noise,
                       const int *step_pre, int max_steps, double dt, int flavor,
                       float *next, double *reward, int *term, int *trunc, int *viol, int *crit, int *ok, int *mask)
{
    const oracle_spec_t *sp = &SPECS[env];
    for (int i = 0; i < n; i++) {
        oracle_step_out_t o;
        oracle_step(env, states + (size_t)i * sp->state_dim, actions + (size_t)i * sp->action_dim,
                    noise ? noise + (size_t)i * sp->k_step : NULL, step_pre[i], max_steps, dt, flavor,
                    next + (size_t)i * sp->state_dim, &o);
        reward[i] = o.reward; term[i] = o.terminated; trunc[i] = o.truncated;
        viol[i] = o.violation_count; crit[i] = o.critical_violations;
        for (int k = 0; k < 3; k++) ok[i * 3 + k] = o.ok[k];
        if (mask) mask[i] = o.viol_mask | (o.shutdown << 8);
    }
}

/* ------------------------------------------------------------------------------
 * Synthetic input generator "nig-philox-v2" (DESIGN.md).  NOT part of the reference
 * (which draws from NumPy's global MT19937): it is the workload generator that
 * bench.py and the full-size parity tests use on both the CPU and the GPU side.
 * Independent restatement of the spec; the product has its own implementation.
 * ---------------------------------------------------------------------------- */
/* Philox4x32 with `rounds` rounds (Random123): the generator uses PHILOX_ROUNDS = 7 since "nig-philox-v2" */
#define PHILOX_ROUNDS 7
static void philox4x32_r(int rounds, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t *out)
{
    for (int r = 0; r < rounds; r++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

#define STREAM_STEP 0u
#define STREAM_RESET 0x40000000u
#define STREAM_ACTION 0x80000000u

/* One standard normal per 32-bit word: piecewise-cubic inverse normal CDF over generated data
 * (nig_probit_table.inc, see neorl-industrial-gym_amd/csrc/gen_probit_table.py): bit 31 = sign,
 * next 23 bits m -> f = m + 0.5; piece = f's float32 exponent and top 5 mantissa bits, position =
 * low 18 mantissa bits taken as an integer p; z = c0 + p(c1' + p(c2' + p c3')) in float32 with the table's
 * pre-scaled coefficients (c1' = c1 2^-18, ...), Horner in three fused multiply-adds. */
static const float PROBIT[768][4] = {
#include "nig_probit_table.inc"
};

static float probit_normal(uint32_t word)
{
    uint32_t v = word >> 8;
    union { float f; uint32_t u; } q;
    q.f = (float)(v & 0x7FFFFFu) + 0.5f;
    const float *c = PROBIT[(q.u >> 18) - (126u << 5)];
    float t = (float)(q.u & 0x3FFFFu);       /* the position's 2^-18 is folded into the table (tests/probit_scale_check.c: same bits) */
    float z = fmaf(c[3], t, c[2]);
    z = fmaf(z, t, c[1]);
    z = fmaf(z, t, c[0]);
    return (v & 0x800000u) ? -z : z;
}

static double u01(uint32_t x) { return (double)(x >> 8) * (1.0 / 16777216.0); }  /* [0,1) */

/* n standard normals for (env_index, t) on a stream: one word each, four per Philox block */
static void gen_normals(uint64_t seed, uint64_t env_index, uint32_t t, uint32_t stream, int n, float *z)
{
    uint32_t x[4];
    for (int j = 0; 4 * j < n; j++) {
        philox4x32_r(PHILOX_ROUNDS, (uint32_t)env_index, (uint32_t)(env_index >> 32), t, stream + (uint32_t)j,
                      (uint32_t)seed, (uint32_t)(seed >> 32), x);
        for (int i = 0; i < 4 && 4 * j + i < n; i++) z[4 * j + i] = probit_normal(x[i]);
    }
}

static void gen_uniforms(uint64_t seed, uint64_t env_index, uint32_t t, uint32_t stream, int n, double *u)
{
    uint32_t x[4];
    for (int j = 0; 4 * j < n; j++) {
        philox4x32_r(PHILOX_ROUNDS, (uint32_t)env_index, (uint32_t)(env_index >> 32), t, stream + (uint32_t)j,
                      (uint32_t)seed, (uint32_t)(seed >> 32), x);
        for (int i = 0; i < 4 && 4 * j + i < n; i++) u[4 * j + i] = u01(x[i]);
    }
}

/* step noise in the reference's draw order; fast-mode value = float32 product sd * z, widened to double */
void oracle_gen_step_noise(int env, uint64_t seed, uint64_t env_index, uint32_t t, double *noise)
{
    float z[24];
    if (env == ORACLE_CR) {                                    /* chemical_reactor.py:149,159 */
        /* two draws per step: launch counters 2k-1 and 2k share one Philox block (counter word k),
         * words 0-1 for the odd counter, 2-3 for the even one */
        gen_normals(seed, env_index, (t + 1u) >> 1, STREAM_STEP, 4, z);
        const float *zz = z + 2 * (1u - (t & 1u));
        noise[0] = (double)(0.1f * zz[0]);                      /* fast-mode step noise: float32 product sd * z */
        noise[1] = (double)(500.0f * zz[1]);
    } else if (env == ORACLE_PG) {                             /* power_grid.py:136,140,144 */
        gen_normals(seed, env_index, t, STREAM_STEP, 23, z);
        for (int i = 0; i < 8; i++) noise[i] = (double)(0.005f * z[i]);
        for (int i = 0; i < 8; i++) noise[8 + i] = (double)z[8 + i];
        for (int i = 0; i < 7; i++) noise[16 + i] = (double)(2.0f * z[16 + i]);
    } else if (env >= ORACLE_SPEC0) {
        const spec_plant_t *P = &SPEC_PLANTS[env - ORACLE_SPEC0];
        /* plant model "v2" (0.4.0): ChemicalReactor's rule -- counters 2k-1, 2k share the block of counter word k */
        gen_normals(seed, env_index, (t + 1u) >> 1, STREAM_STEP, 4, z);
        const float *zz = z + 2 * (1u - (t & 1u));
        noise[0] = (double)(P->nsd[0] * zz[0]);
        noise[1] = (double)(P->nsd[1] * zz[1]);
    }
}

void oracle_gen_reset_noise(int env, uint64_t seed, uint64_t env_index, uint32_t t, double *noise)
{
    float z[24];
    double u[8];
    if (env == ORACLE_CR) {                                    /* chemical_reactor.py:93-103 */
        /* "nig-philox-v2": the fast-mode draw is the float32 product sd * z (as the step noise has been since v1), handed
         * to _get_initial_state's fp64 "mean + draw" as the double it is */
        static const float sc[8] = {2.0f, 10000.0f, 5.0f, 3.0f, 0.1f, 2.0f, 1.0f, 5.0f};
        gen_normals(seed, env_index, t, STREAM_RESET, 8, z);
        for (int i = 0; i < 8; i++) noise[i] = (double)(sc[i] * z[i]);
    } else if (env == ORACLE_PG) {                             /* power_grid.py:98-108 */
        /* "nig-philox-v2": float32 draws -- normals sd * z, the load factor fma(0.4, u, -0.2) with u the 24-bit uniform
         * (exact in float32) -- handed to _get_initial_state's fp64 arithmetic as doubles.  (float)(1.0 + d), (float)(base + d)
         * and (float)(base * (1.0 + d)) are then exact-in-double sums / products rounded once: on the device one
         * v_add_f32 / v_fma_f32 each. */
        /* "nig-philox-v3" (round 4): the eight load factors are 16-bit uniforms k / 65536 taken from the LOW BYTES of the reset
         * normals' words -- block b < 4 of the reset stream carries factors 2 b (byte 0 of words 0, 1) and 2 b + 1 (words 2, 3) --
         * instead of two more Philox blocks (v2: STREAM_RESET + 16 / + 17).  k / 65536 = (k << 8) / 2^24 is one of v2's 24-bit
         * uniforms, so the exactness statements above are unchanged. */
        gen_normals(seed, env_index, t, STREAM_RESET, 23, z);
        for (int b = 0; b < 4; b++) {
            uint32_t x[4];
            philox4x32_r(PHILOX_ROUNDS, (uint32_t)env_index, (uint32_t)(env_index >> 32), t, STREAM_RESET + (uint32_t)b,
                          (uint32_t)seed, (uint32_t)(seed >> 32), x);
            for (int q = 0; q < 2; q++) {
                const uint32_t k16 = (x[2 * q] & 0xFFu) | ((x[2 * q + 1] & 0xFFu) << 8);
                noise[16 + 2 * b + q] = (double)fmaf(0.4f / 65536.0f, (float)k16, -0.2f);
            }
        }
        (void)u;
        for (int i = 0; i < 8; i++) noise[i] = (double)(0.01f * z[i]);
        for (int i = 0; i < 8; i++) noise[8 + i] = (double)(2.0f * z[8 + i]);
        for (int i = 0; i < 7; i++) noise[24 + i] = (double)(10.0f * z[16 + i]);
    } else if (env == ORACLE_RA) {                             /* robot_assembly.py:118-122 */
        gen_uniforms(seed, env_index, t, STREAM_RESET, 7, u);
        const double lo = -RA_PI * 0.5, hi = RA_PI * 0.5;
        for (int i = 0; i < 7; i++) noise[i] = lo + (hi - lo) * u[i];
    } else if (env >= ORACLE_SPEC0) {
        const spec_plant_t *P = &SPEC_PLANTS[env - ORACLE_SPEC0];
        gen_normals(seed, env_index, t, STREAM_RESET, P->np, z);
        for (int i = 0; i < P->np; i++) noise[i] = 0.0 + (double)P->sd0[i] * (double)z[i];
    }
}

/* uniform float32 actions in [-1, 1): 2*u - 1 with u a 24-bit uniform (exact in float32) */
void oracle_gen_actions(int env, uint64_t seed, uint64_t env_index, uint32_t t, float *a)
{
    double u[12];
    gen_uniforms(seed, env_index, t, STREAM_ACTION, SPECS[env].action_dim, u);
    for (int i = 0; i < SPECS[env].action_dim; i++)
        a[i] = (float)((double)act_low(env, i) + ((double)act_high(env, i) - (double)act_low(env, i)) * u[i]);
}

/* ------------------------------------------------------------------------------
 * Free-running rollout driver (auto-reset), used as (1) the exact cross-check for the
 * device "fast mode" and (2) bench.py's cpu_baseline.  Mirrors the loop shape of the
 * reference's benchmark_environment_steps (performance_benchmark.py:106-133):
 * sample action -> step -> reset on done.  Env i uses global index env0 + i.
 *
 * Per-env outputs after T steps (arrays of n): final state [n][S] row-major,
 * int64 sums: steps, episodes finished, violation_count, critical_violations,
 * terminated count, truncated count; double sum of rewards.
 * ---------------------------------------------------------------------------- */
typedef struct {
    int64_t steps, episodes, violations, critical, terminated, truncated;
    double reward_sum;
} oracle_tally_t;

void oracle_rollout(int env, int64_t n, uint64_t env0, uint64_t seed, uint32_t t0, int T,
                    int max_steps, double dt, int flavor, int nthreads,
                    float *state_io /* [n][S] in: ignored if init!=0 */, int32_t *step_io /* [n] */,
                    int init, oracle_tally_t *tally /* [n] or NULL */, oracle_tally_t *total)
{
    const oracle_spec_t *sp = &SPECS[env];
    const int S = sp->state_dim;
    oracle_tally_t tot; memset(&tot, 0, sizeof tot);
    (void)nthreads;
#ifdef _OPENMP
#pragma omp parallel num_threads(nthreads > 0 ? nthreads : 1)
#endif
    {
        oracle_tally_t loc; memset(&loc, 0, sizeof loc);
#ifdef _OPENMP
#pragma omp for schedule(static)
#endif
        for (int64_t i = 0; i < n; i++) {
            float s[32], nx[32], a[16];
            double nz[32];
            uint64_t gi = env0 + (uint64_t)i;
            int step;
            oracle_tally_t me; memset(&me, 0, sizeof me);
            if (init) {
                oracle_gen_reset_noise(env, seed, gi, t0, nz);
                oracle_reset(env, nz, flavor, s);
                step = 0;
            } else {
                memcpy(s, state_io + (size_t)i * S, S * sizeof(float));
                step = step_io[i];
            }
            for (int k = 0; k < T; k++) {
                uint32_t t = t0 + 1u + (uint32_t)k;
                oracle_step_out_t o;
                oracle_gen_actions(env, seed, gi, t, a);
                oracle_gen_step_noise(env, seed, gi, t, nz);
                oracle_step(env, s, a, nz, step, max_steps, dt, flavor, nx, &o);
                me.steps++; me.violations += o.violation_count; me.critical += o.critical_violations;
                me.reward_sum += o.reward;
                me.terminated += o.terminated; me.truncated += (o.truncated && !o.terminated);
                if (o.terminated || o.truncated) {
                    me.episodes++;
                    oracle_gen_reset_noise(env, seed, gi, t, nz);
                    oracle_reset(env, nz, flavor, s);
                    step = 0;
                } else {
                    memcpy(s, nx, S * sizeof(float));
                    step++;
                }
            }
            memcpy(state_io + (size_t)i * S, s, S * sizeof(float));
            step_io[i] = step;
            if (tally) tally[i] = me;
            loc.steps += me.steps; loc.episodes += me.episodes; loc.violations += me.violations;
            loc.critical += me.critical; loc.terminated += me.terminated; loc.truncated += me.truncated;
            loc.reward_sum += me.reward_sum;
        }
#ifdef _OPENMP
#pragma omp critical
#endif
        {
            tot.steps += loc.steps; tot.episodes += loc.episodes; tot.violations += loc.violations;
            tot.critical += loc.critical; tot.terminated += loc.terminated; tot.truncated += loc.truncated;
            tot.reward_sum += loc.reward_sum;
        }
    }
    if (total) *total = tot;
}


/* ------------------------------------------------------------------------------
 * On-device policy "nig-policy-v1" (include/nig.h): independent restatement for the
 * closed-loop cross-checks.  Policy families = the reference's non-neural agents
 * (benchmarks/baseline_agents.py:28-114) and get_dataset behaviour policies
 * (chemical_reactor.py:364-393, power_grid.py:216-233, robot_assembly.py:266-290).
 * ---------------------------------------------------------------------------- */
#define STREAM_POLICY 0xC0000000u
typedef struct {
    int32_t kind; uint32_t colmask;
    float Wt[32][10]; float b[10]; float sigma[10]; float half_range[10];
    float p_uniform, uniform_range, clip_lo, clip_hi, kp, ki, kd; float setpoint[10];
} oracle_policy_t;

static float u01f(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }

static void policy_action(int env, const oracle_policy_t *P, const float *obs, uint64_t seed, uint64_t gi, uint32_t t,
                          float *integ, float *eprev, float *u)
{
    const int S = SPECS[env].state_dim, A = SPECS[env].action_dim;
    if (P->kind == 2) {                                        /* PID, baseline_agents.py:61-80 */
        for (int j = 0; j < A; j++) {
            float e = P->setpoint[j] - obs[j];
            integ[j] = integ[j] + e;
            u[j] = (P->kp * e + P->ki * integ[j]) + P->kd * (e - eprev[j]);
            eprev[j] = e;
        }
    } else {
        for (int j = 0; j < A; j++) u[j] = P->b[j];
        for (int k = 0; k < S; k++) {
            int nz = 0;
            for (int j = 0; j < A; j++) if (P->Wt[k][j] != 0.0f) nz = 1;
            if (!nz) continue;                                 /* zero columns are skipped */
            for (int j = 0; j < A; j++) u[j] = u[j] + P->Wt[k][j] * obs[k];
        }
    }
    int any_sigma = 0, any_half = 0;
    for (int j = 0; j < A; j++) { if (P->sigma[j] != 0.0f) any_sigma = 1; if (P->half_range[j] != 0.0f) any_half = 1; }
    uint32_t x[4];
    if (any_sigma) {
        float z[12];
        gen_normals(seed, gi, t, STREAM_POLICY + 1u, A, z);
        for (int j = 0; j < A; j++) u[j] = u[j] + P->sigma[j] * z[j];
    }
    if (any_half) {
        for (int b4 = 0; 4 * b4 < A; b4++) {
            philox4x32_r(PHILOX_ROUNDS, (uint32_t)gi, (uint32_t)(gi >> 32), t, STREAM_POLICY + 8u + (uint32_t)b4, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            for (int i = 0; i < 4 && 4 * b4 + i < A; i++)
                u[4 * b4 + i] = u[4 * b4 + i] + P->half_range[4 * b4 + i] * (2.0f * u01f(x[i]) - 1.0f);
        }
    }
    if (P->p_uniform > 0.0f) {
        philox4x32_r(PHILOX_ROUNDS, (uint32_t)gi, (uint32_t)(gi >> 32), t, STREAM_POLICY, (uint32_t)seed, (uint32_t)(seed >> 32), x);
        int rnd = u01f(x[0]) < P->p_uniform;
        for (int b4 = 0; 4 * b4 < A; b4++) {
            philox4x32_r(PHILOX_ROUNDS, (uint32_t)gi, (uint32_t)(gi >> 32), t, STREAM_POLICY + 16u + (uint32_t)b4, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            for (int i = 0; i < 4 && 4 * b4 + i < A; i++) {
                float ra = P->uniform_range * (2.0f * u01f(x[i]) - 1.0f);
                if (rnd) u[4 * b4 + i] = ra;
            }
        }
    }
    for (int j = 0; j < A; j++) {
        float v = u[j];
        v = (v < P->clip_lo) ? P->clip_lo : v;
        v = (v > P->clip_hi) ? P->clip_hi : v;
        u[j] = v;
    }
}

/* Closed-loop rollout: action = policy(obs) -> step; lanes freeze at done unless autoreset.
 * Optional trajectories (row-major): obs_pre [T][n][S], act [T][n][A], reward [T][n] (double),
 * live [T][n] (1 where the lane took the step). */
void oracle_rollout_policy(int env, int64_t n, uint64_t env0, uint64_t seed, uint32_t t0, int T,
                           int max_steps, double dt, int flavor, int autoreset, const oracle_policy_t *P,
                           float *state_out /* [n][S] */, int32_t *step_out, int32_t *done_out,
                           oracle_tally_t *tally /* [n] */, double *ep_return_last /* [n] last finished */,
                           float *obs_pre, float *act, double *reward, uint8_t *live)
{
    const oracle_spec_t *sp = &SPECS[env];
    const int S = sp->state_dim, A = sp->action_dim;
    for (int64_t i = 0; i < n; i++) {
        float s[32], nx[32], a[12], integ[12] = {0}, eprev[12] = {0};
        double nz[32];
        uint64_t gi = env0 + (uint64_t)i;
        oracle_tally_t me; memset(&me, 0, sizeof me);
        oracle_gen_reset_noise(env, seed, gi, t0, nz);
        oracle_reset(env, nz, flavor, s);
        int step = 0, done = 0;
        double ret = 0.0; float ret32 = 0.0f;
        if (ep_return_last) ep_return_last[i] = 0.0;
        for (int k = 0; k < T; k++) {
            uint32_t t = t0 + 1u + (uint32_t)k;
            if (live) live[(size_t)k * n + i] = (uint8_t)!done;
            if (done) continue;
            policy_action(env, P, s, seed, gi, t, integ, eprev, a);
            if (obs_pre) memcpy(obs_pre + ((size_t)k * n + i) * S, s, S * sizeof(float));
            if (act) memcpy(act + ((size_t)k * n + i) * A, a, A * sizeof(float));
            oracle_step_out_t o;
            oracle_gen_step_noise(env, seed, gi, t, nz);
            oracle_step(env, s, a, nz, step, max_steps, dt, flavor, nx, &o);
            if (reward) reward[(size_t)k * n + i] = o.reward;
            me.steps++; me.violations += o.violation_count; me.critical += o.critical_violations;
            me.reward_sum += o.reward;
            if (env == ORACLE_CR) { ret32 = ret32 + (float)o.reward; ret = (double)ret32; } else ret += o.reward;
            me.terminated += o.terminated; me.truncated += (o.truncated && !o.terminated);
            if (o.terminated || o.truncated) {
                me.episodes++;
                if (ep_return_last) ep_return_last[i] = ret;
                ret = 0.0; ret32 = 0.0f;
                if (autoreset) {
                    oracle_gen_reset_noise(env, seed, gi, t, nz);
                    oracle_reset(env, nz, flavor, s);
                    step = 0;
                } else {
                    memcpy(s, nx, S * sizeof(float));
                    step++; done = 1;
                }
            } else {
                memcpy(s, nx, S * sizeof(float));
                step++;
            }
        }
        memcpy(state_out + (size_t)i * S, s, S * sizeof(float));
        step_out[i] = step; done_out[i] = done;
        if (tally) tally[i] = me;
    }
}


/* ------------------------------------------------------------------------------
 * MLP actor (S -> 256 -> 256 -> A, ReLU, tanh; agents/networks.py:47-70,125-144) in the exact
 * float32 fma-chain order of the device's MFMA evaluation (v_mfma_f32_32x32x2_f32 is
 * fma(a1,b1, fma(a0,b0, c)) per k-step): layer 1 in natural k order, layers 2/3 in the order an
 * accumulator tile exposes its rows (register t of a 32-row tile: rows rho(t), rho(t)+4 with
 * rho(t) = (t&3) + 8(t>>2)), the bias as a last k-step (fma(b,1,acc), then fma(0,0,acc)).
 * W are row-major [in][out] (Flax Dense kernel layout).
 * ---------------------------------------------------------------------------- */
#define MLP_H 256
static int mlp_rho(int t) { return (t & 3) + 8 * (t >> 2); }

/* the network up to its head's pre-activations pre[0..A): D inputs x (an odd D is padded with one zero input, as the
 * device's operand stream pads it: MLP_CDIM), layers 1 / 2 / head in the device's summation order */
static void mlp_pre(int D, int A, const float *W1, const float *b1, const float *W2, const float *b2,
                    const float *W3, const float *b3, const float *x, float *pre)
{
    float h1[MLP_H], h2[MLP_H];
    for (int u = 0; u < MLP_H; u++) {
        float acc = 0.0f;
        for (int ks = 0; 2 * ks < D; ks++) {
            acc = fmaf(W1[(size_t)(2 * ks) * MLP_H + u], x[2 * ks], acc);
            acc = (2 * ks + 1 < D) ? fmaf(W1[(size_t)(2 * ks + 1) * MLP_H + u], x[2 * ks + 1], acc) : fmaf(0.0f, 0.0f, acc);
        }
        acc = fmaf(b1[u], 1.0f, acc); acc = fmaf(0.0f, 0.0f, acc);
        h1[u] = fmaxf(acc, 0.0f);
    }
    for (int v = 0; v < MLP_H; v++) {
        float acc = 0.0f;
        for (int kt = 0; kt < MLP_H / 32; kt++)
            for (int t = 0; t < 16; t++) {
                int k0 = 32 * kt + mlp_rho(t), k1 = k0 + 4;
                acc = fmaf(W2[(size_t)k0 * MLP_H + v], h1[k0], acc);
                acc = fmaf(W2[(size_t)k1 * MLP_H + v], h1[k1], acc);
            }
        acc = fmaf(b2[v], 1.0f, acc); acc = fmaf(0.0f, 0.0f, acc);
        h2[v] = fmaxf(acc, 0.0f);
    }
    for (int j = 0; j < A; j++) {
        /* the head runs on K = 1 MFMAs on the device (nig_kernels.hpp: v_mfma_f32_4x4x1 for at most four actions,
         * v_mfma_f32_16x16x1 above): each lane half sums the hidden rows its accumulator registers hold -- half 0 rows
         * rho(t), half 1 rows rho(t) + 4 -- as its own fma chain, the bias record is fma(b, 1, .) on half 0 and
         * fma(b, 0, .) on half 1, one float32 add joins the halves */
        float acc0 = 0.0f, acc1 = 0.0f;
        for (int kt = 0; kt < MLP_H / 32; kt++)
            for (int t = 0; t < 16; t++) {
                int k0 = 32 * kt + mlp_rho(t), k1 = k0 + 4;
                acc0 = fmaf(W3[(size_t)k0 * A + j], h2[k0], acc0);
                acc1 = fmaf(W3[(size_t)k1 * A + j], h2[k1], acc1);
            }
        acc0 = fmaf(b3[j], 1.0f, acc0); acc1 = fmaf(b3[j], 0.0f, acc1);
        pre[j] = acc0 + acc1;
    }
}

static void mlp_actor(int S, int A, const float *W1, const float *b1, const float *W2, const float *b2,
                      const float *W3, const float *b3, const float *obs, int flavor, float *act)
{
    float pre[16];
    (void)flavor;
    mlp_pre(S, A, W1, b1, W2, b2, W3, b3, obs, pre);
    for (int j = 0; j < A; j++) act[j] = det_tanhf(pre[j]);
}

void oracle_mlp_actions(int env, int64_t n, const float *W1, const float *b1, const float *W2, const float *b2,
                        const float *W3, const float *b3, const float *obs, float *act)
{
    const int S = SPECS[env].state_dim, A = SPECS[env].action_dim;
    for (int64_t i = 0; i < n; i++) mlp_actor(S, A, W1, b1, W2, b2, W3, b3, obs + (size_t)i * S, MATH_POLY, act + (size_t)i * A);
}

/* the actor's head pre-activations (the argument of its tanh), bit for bit what the device's head forms */
void oracle_mlp_preact(int env, int64_t n, const float *W1, const float *b1, const float *W2, const float *b2,
                       const float *W3, const float *b3, const float *obs, float *pre)
{
    const int S = SPECS[env].state_dim, A = SPECS[env].action_dim;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) mlp_pre(S, A, W1, b1, W2, b2, W3, b3, obs + (size_t)i * S, pre + (size_t)i * A);
}

/* the safety critic of nig_rollout_mlp_safe: p = sigmoid(critic([s, a, 0-pad])), critic (S + A) -> 256 -> 256 -> 1 in
 * the device's order -- layer 1 on x = [s, a] in natural k order, layer 2 as the actor's, the one-row head as two lane-half
 * fma chains joined by one add (the actor's K = 1 head with A = 1; nig_api.hip nig_set_mlp_safety) */
#define MLP_CRITIC_MAXIN 50      /* the device's limit on the critic's input: an even S <= 34 (its MFMA layer 1) + A <= 16 */
int oracle_mlp_critic(int env, int64_t n, const float *C1, const float *c1, const float *C2, const float *c2,
                      const float *C3, const float *c3, const float *obs, const float *act, float *prob)
{
    const int S = SPECS[env].state_dim, A = SPECS[env].action_dim;
    if (S + A > MLP_CRITIC_MAXIN) return -1;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) {
        float x[MLP_CRITIC_MAXIN], z;
        memcpy(x, obs + (size_t)i * S, S * sizeof(float));
        memcpy(x + S, act + (size_t)i * A, A * sizeof(float));
        mlp_pre(S + A, 1, C1, c1, C2, c2, C3, c3, x, &z);
        prob[i] = det_sigmoidf(z);
    }
    return 0;
}

/* closed loop with the MLP actor (same conventions as oracle_rollout_policy) */
void oracle_rollout_mlp(int env, int64_t n, uint64_t env0, uint64_t seed, uint32_t t0, int T, int max_steps, double dt,
                        int flavor, int autoreset, int nthreads, const float *W1, const float *b1, const float *W2,
                        const float *b2, const float *W3, const float *b3, float *state_out, int32_t *step_out,
                        int32_t *done_out, oracle_tally_t *tally, float *act_traj /* [T][n][A] or NULL */)
{
    const oracle_spec_t *sp = &SPECS[env];
    const int S = sp->state_dim, A = sp->action_dim;
    (void)nthreads;
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(nthreads > 0 ? nthreads : 1)
#endif
    for (int64_t i = 0; i < n; i++) {
        float s[32], nx[32], a[16];
        double nz[32];
        uint64_t gi = env0 + (uint64_t)i;
        oracle_tally_t me; memset(&me, 0, sizeof me);
        oracle_gen_reset_noise(env, seed, gi, t0, nz);
        oracle_reset(env, nz, flavor, s);
        int step = 0, done = 0;
        for (int k = 0; k < T; k++) {
            uint32_t t = t0 + 1u + (uint32_t)k;
            if (done) continue;
            mlp_actor(S, A, W1, b1, W2, b2, W3, b3, s, flavor, a);
            if (act_traj) memcpy(act_traj + ((size_t)k * n + i) * A, a, A * sizeof(float));
            oracle_step_out_t o;
            oracle_gen_step_noise(env, seed, gi, t, nz);
            oracle_step(env, s, a, nz, step, max_steps, dt, flavor, nx, &o);
            me.steps++; me.violations += o.violation_count; me.critical += o.critical_violations; me.reward_sum += o.reward;
            me.terminated += o.terminated; me.truncated += (o.truncated && !o.terminated);
            if (o.terminated || o.truncated) {
                me.episodes++;
                if (autoreset) { oracle_gen_reset_noise(env, seed, gi, t, nz); oracle_reset(env, nz, flavor, s); step = 0; }
                else { memcpy(s, nx, S * sizeof(float)); step++; done = 1; }
            } else { memcpy(s, nx, S * sizeof(float)); step++; }
        }
        memcpy(state_out + (size_t)i * S, s, S * sizeof(float));
        step_out[i] = step; done_out[i] = done;
        if (tally) tally[i] = me;
    }
}

void oracle_policy_action(int env, const oracle_policy_t *P, const float *obs, uint64_t seed, uint64_t gi, uint32_t t,
                          float *integ, float *eprev, float *u)
{
    policy_action(env, P, obs, seed, gi, t, integ, eprev, u);
}

/* exposed for unit tests of the math layer */
float oracle_det_expf(float x) { return det_expf(x); }
float oracle_det_logf(float x) { return det_logf(x); }
float oracle_probit_normal(uint32_t word) { return probit_normal(word); }
void oracle_det_sincos(double x, double *s, double *c) { det_sincos(x, s, c); }
void oracle_philox_rounds(const uint32_t *ctr, const uint32_t *key, int rounds, uint32_t *out)   /* known-answer tests */
{
    philox4x32_r(rounds, ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
}

void oracle_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out)
{
    philox4x32_r(PHILOX_ROUNDS, ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
}
void oracle_gen_normals(uint64_t seed, uint64_t env_index, uint32_t t, uint32_t stream, int n, float *z)
{
    gen_normals(seed, env_index, t, stream, n, z);
}

/* ------------------------------------------------------------------------------
 * Batch exports of the math layer for the device-vs-oracle tests (tests/test_gpu_detmath.py) and the accuracy
 * sweeps (tests/detmath_check.c): OpenMP-parallel, as many threads as OMP_NUM_THREADS asks for.
 * ---------------------------------------------------------------------------- */
/* the device's constant division (csrc/nig_detmath.hpp fdiv_c) restated: the three rounded steps (x 2^-64 and the
 * quotient scaled back for |x| >= 2^64 when c < 1) and v_div_fixup's result for a finite divisor c > 0 whose exponent
 * is within 150 of every float's: NaN stays NaN, x = +-inf gives +-inf, x = +-0 gives +-0, otherwise |q| with x's sign */
static float fdiv_c_seq(float x, float c)
{
    volatile float rcv = 1.0f / c;
    const float rc = rcv;
    if (x != x) return x;
    if (isinf(x) || x == 0.0f) return x;
    const int big = c < 1.0f && fabsf(x) >= 0x1p64f;
    const float xs = big ? x * 0x1p-64f : x;
    const float q0 = xs * rc;
    const float r = fmaf(-c, q0, xs);
    float q = fmaf(r, rc, q0);
    q = big ? q * 0x1p64f : q;
    return copysignf(fabsf(q), x);
}

enum { DM_EXPF, DM_LOGF, DM_TANHF, DM_SIGMOIDF, DM_SINF };
static float dm_unary(int fn, float x)
{
    switch (fn) {
    case DM_EXPF: return det_expf(x);
    case DM_LOGF: return det_logf(x);
    case DM_TANHF: return det_tanhf(x);
    case DM_SIGMOIDF: return det_sigmoidf(x);
    default: return det_sinf(x);
    }
}
static int same_f32(float a, float b)
{
    uint32_t ua, ub;
    memcpy(&ua, &a, 4); memcpy(&ub, &b, 4);
    return ua == ub || (a != a && b != b);       /* NaNs compare as "both NaN": x86 and gfx950 make different default NaNs */
}

void oracle_det_expf_batch(const float *x, float *y, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) y[i] = det_expf(x[i]);
}
void oracle_det_logf_batch(const float *x, float *y, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) y[i] = det_logf(x[i]);
}
void oracle_det_tanhf_batch(const float *x, float *y, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) y[i] = det_tanhf(x[i]);
}
void oracle_det_sigmoidf_batch(const float *x, float *y, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) y[i] = det_sigmoidf(x[i]);
}
void oracle_det_sinf_batch(const float *x, float *y, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) y[i] = det_sinf(x[i]);
}
void oracle_det_powf_batch(const float *x, const float *y, float *z, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) z[i] = det_powf(x[i], y[i]);
}
void oracle_fdiv_c_batch(float c, const float *x, float *y, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) y[i] = fdiv_c_seq(x[i], c);
}
void oracle_det_exp_batch(const double *x, double *y, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) y[i] = det_exp64(x[i]);
}
void oracle_det_sincos_batch(const double *x, double *s, double *c, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) det_sincos(x[i], s + i, c + i);
}
/* csrc/nig_detmath.hpp ddiv_y without v_div_fixup (the caller's operands are finite and nonzero) */
void oracle_ddiv_y_batch(const double *a, const double *b, const double *y, double *q, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) {
        const double q0 = a[i] * y[i];
        const double q1 = fma(fma(-q0, b[i], a[i]), y[i], q0);
        q[i] = fma(fma(-q1, b[i], a[i]), y[i], q1);
    }
}
void oracle_probit_normal_batch(const uint32_t *w, float *z, int64_t n)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) z[i] = probit_normal(w[i]);
}
void oracle_philox_batch(const uint32_t *ctr, const uint32_t *key, uint32_t *out, int64_t n)   /* [n][4], [n][2], [n][4] */
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++)
        philox4x32_r(PHILOX_ROUNDS, ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1], out + 4 * i);
}

/* device output got[i] of unary function fn at x = the float with bits base + i, against the oracle: the number of
 * words that differ (NaN == NaN), the first such i in *first (-1 if none) */
int64_t oracle_cmp_unary_f32(int fn, uint32_t base, int64_t n, const float *got, int64_t *first)
{
    int64_t bad = 0, lo = INT64_MAX;
#pragma omp parallel for schedule(static) reduction(+:bad) reduction(min:lo)
    for (int64_t i = 0; i < n; i++) {
        const uint32_t b = base + (uint32_t)i;
        float x;
        memcpy(&x, &b, 4);
        if (!same_f32(dm_unary(fn, x), got[i])) { bad++; if (i < lo) lo = i; }
    }
    *first = bad ? lo : -1;
    return bad;
}

/* device outputs got[i] of fdiv_c(x, c) at x = bits base + i against the restated sequence (fdiv_c_seq): the number of
 * words that differ (NaN == NaN), the first such i in *first (-1 if none) */
int64_t oracle_cmp_fdiv_c(float c, uint32_t base, int64_t n, const float *got, int64_t *first)
{
    int64_t bad = 0, lo = INT64_MAX;
#pragma omp parallel for schedule(static) reduction(+:bad) reduction(min:lo)
    for (int64_t i = 0; i < n; i++) {
        const uint32_t b = base + (uint32_t)i;
        float x;
        memcpy(&x, &b, 4);
        if (!same_f32(fdiv_c_seq(x, c), got[i])) { bad++; if (i < lo) lo = i; }
    }
    *first = bad ? lo : -1;
    return bad;
}
