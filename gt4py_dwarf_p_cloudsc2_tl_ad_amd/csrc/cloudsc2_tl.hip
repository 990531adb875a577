// cloudsc2_tl as a hand-written CDNA4 kernel: NL trajectory + tangent-linear perturbation in one
// forward sweep.  Restates
// /root/reference/src/cloudsc2_gt4py/physics/tangent_linear/_stencils/cloudsc2.py:124-774 and
// /root/reference/src/cloudsc2_gt4py/physics/tangent_linear/_stencils/cuadjtqs.py:22-84
// (line numbers below refer to the first file).  Same execution model as cloudsc2_nl.hip: one lane
// per column, carried state (rfl, sfl, covptot and their perturbations) in registers, level k+1
// prefetched while level k is computed, flux shift fused into the sweep.
//
// Template flags: REG = LREGCL (regularisations :294-301, :367-368, :444-448, :475-487, :667-668);
// EVAP = LEVAPLS2 or LDRAIN1D (precipitation-evaporation block :528-616 and the 1.9 RCLCRIT / 1e-4
// autoconversion thresholds; never enabled by the reference's own drivers).
#include "cloudsc2_launch.hpp"

#ifndef CS2_TL_DIAG
#define CS2_TL_DIAG 0   // diagnostics only (wrong results): 1 = the kernel's memory traffic without the physics
#endif

namespace cs2 {

template <typename T>
struct TLCarry {
    T rfl, rfl_i, sfl, sfl_i, covptot, covptot_i, aph_k, aph_k_i;
    T aph_s, aph_s_i;  // surface pressure and its perturbation (:126-127), read by the evaporation block only
};

template <typename T>
struct TLOut {
    T clc, clc_i, tnd_q, tnd_q_i, tnd_t, tnd_t_i, tnd_ql, tnd_ql_i, tnd_qi, tnd_qi_i, rfln, rfln_i, sfln, sfln_i;
    T covptot, covptot_i;  // :185-186, non-zero only where the evaporation block ran (:586-587)
};

// One iteration of tangent_linear/_stencils/cuadjtqs.py:22-52 with shared reciprocals
// (rap = 1/ap from the caller, r = 1/(t - z4es) serves the exponent, foeew_i, z2s and z2s_i).
template <typename T>
__device__ __forceinline__ void tl_cuadj_iter(const Ext<T>& e, const ExpK<T>& xk, T rap, T ap_i, T& t, T& t_i, T& q,
                                              T& q_i, T z3es, T z4es, T z5alcp, T zaldcp) {
    const T qp_i = -ap_i * rap * rap;
    const T r = frcp<T>(t - z4es);
    const T foeew = e.R2ES * fexp<T>(xk, z3es * (t - e.RTT) * r);
    const T foeew_i = foeew * z3es * t_i * (e.RTT - z4es) * r * r;
    T qsat = rap * foeew;
    T qsat_i = qp_i * foeew + rap * foeew_i;
    if (qsat > e.ZQMAX) {
        qsat = e.ZQMAX;
        qsat_i = T(0.0);
    }
    const T cor = frcp<T>(T(1.0) - e.RETV * qsat);
    const T cor_i = e.RETV * qsat_i * cor * cor;
    qsat_i = qsat_i * cor + qsat * cor_i;
    qsat *= cor;
    const T z2s = z5alcp * r * r;
    const T z2s_i = T(-2.0) * z5alcp * t_i * r * r * r;
    const T rden = frcp<T>(T(1.0) + qsat * cor * z2s);
    const T cond = (q - qsat) * rden;
    const T cond_i = (q_i - qsat_i) * rden -
                     (q - qsat) * (qsat_i * cor * z2s + qsat * cor_i * z2s + qsat * cor * z2s_i) * rden * rden;
    t += zaldcp * cond;
    t_i += zaldcp * cond_i;
    q -= cond;
    q_i -= cond_i;
}

// One level of the forward sweep (:149-753) for one column.  x = trajectory inputs, y = perturbations.
// Same algebra as the reference; divisions are x * frcp(y) with shared reciprocals, tanh/cosh come
// from ONE exponential: with ex = exp(-0.34 (t - RLPTRC)), rr = 1/(1 + ex):
//   0.545 (tanh u + 1) = 1.09 rr,   1 / cosh(u)^2 = 4 ex rr^2      (u = 0.17 (t - RLPTRC)).
template <typename T, bool REG, bool EVAP>
__device__ __forceinline__ TLOut<T> tl_level(const Ext<T>& e, const NLK<T>& kc, const ExpK<T>& xk, const LevelIn<T>& x,
                                             const LevelIn<T>& y, int k, T eta_k, T scalm, const CrhCol<T>& crh, T dt,
                                             TLCarry<T>& c) {
    TLOut<T> o;
#if CS2_TL_DIAG == 1
    {
        const T s1 = x.ap + x.aph1 + x.lu1 + x.lude + x.mfd + x.mfu + x.q + x.qi + x.ql + x.qsat + x.supsat + x.t + x.tq + x.tqi +
                     x.tql + x.tt;
        const T s2 = y.ap + y.aph1 + y.lu1 + y.lude + y.mfd + y.mfu + y.q + y.qi + y.ql + y.qsat + y.supsat + y.t + y.tq + y.tqi +
                     y.tql + y.tt;
        o.clc = s1; o.clc_i = s2; o.tnd_q = s1 + s2; o.tnd_q_i = s1 - s2; o.tnd_t = s1 * s2; o.tnd_t_i = s2 - s1;
        o.tnd_ql = s1 + T(1); o.tnd_ql_i = s2 + T(1); o.tnd_qi = s1 + T(2); o.tnd_qi_i = s2 + T(2);
        o.rfln = c.rfl + s1; o.rfln_i = c.rfl_i + s2; o.sfln = c.sfl + s2; o.sfln_i = c.sfl_i + s1;
        o.covptot = s1 - T(1); o.covptot_i = s2 - T(1);
        c.rfl = o.rfln; c.rfl_i = o.rfln_i; c.sfl = o.sfln; c.sfl_i = o.sfln_i; c.aph_k = x.aph1; c.aph_k_i = y.aph1;
        return o;
    }
#endif
    // :139-140, :151-156
    T t = x.t + dt * x.tt;
    T t_i = y.t + dt * y.tt;
    T q = x.q + dt * x.tq + x.supsat;
    T q_i = y.q + dt * y.tq + y.supsat;
    const T ql = x.ql + dt * x.tql;
    const T ql_i = y.ql + dt * y.tql;
    const T qi = x.qi + dt * x.tqi;
    const T qi_i = y.qi + dt * y.tqi;
    // :171-180
    const T dp = x.aph1 - c.aph_k;
    const T dp_i = y.aph1 - c.aph_k_i;
    const T rdp = frcp<T>(dp);
    const T zden = e.RCPD + e.RCPD * e.RVTMP2 * q;
    const T zz = frcp<T>(zden);
    const T zz_i = -e.RCPD * e.RVTMP2 * q_i * zz * zz;
    const T lfdcp = e.RLMLT * zz, lfdcp_i = e.RLMLT * zz_i;
    const T lsdcp = e.RLSTT * zz, lsdcp_i = e.RLSTT * zz_i;
    const T lvdcp = e.RLVTT * zz, lvdcp_i = e.RLVTT * zz_i;
    // :189-205
    const T rl = frcp<T>(t - e.R4LES);
    const T ri = frcp<T>(t - e.R4IES);
    const T rap = frcp<T>(x.ap);
    T fwat, fwat_i, z3es, z4es, r4;
    if (t < e.RTT) {
        T ex, rr;
        fwat = logistic_fwat<T>(xk, kc.fw2, e.RLPTRC, t, ex, rr);
        fwat_i = T(0.545) * T(0.17) * t_i * logistic_sech2<T>(ex, rr);
        z3es = e.R3IES;
        z4es = e.R4IES;
        r4 = ri;
    } else {
        fwat = T(1.0);
        fwat_i = T(0.0);
        z3es = e.R3LES;
        z4es = e.R4LES;
        r4 = rl;
    }
    const T foeew = e.R2ES * fexp<T>(xk, z3es * (t - e.RTT) * r4);
    const T foeew_i = z3es * (e.RTT - z4es) * t_i * foeew * r4 * r4;
    T esdp = foeew * rap;
    T esdp_i = foeew_i * rap - foeew * y.ap * rap * rap;
    T cor;
    if (esdp > e.ZQMAX) {
        esdp = e.ZQMAX;
        esdp_i = T(0.0);
        cor = kc.cormax;
    } else {
        cor = frcp<T>(T(1.0) - e.RETV * esdp);
    }
    // :207-222
    const T facw = e.R5LES * rl * rl;
    const T facw_i = T(-2.0) * e.R5LES * t_i * rl * rl * rl;
    const T faci = e.R5IES * ri * ri;
    const T faci_i = T(-2.0) * e.R5IES * t_i * ri * ri * ri;
    const T fac = fwat * facw + (T(1.0) - fwat) * faci;
    const T fac_i = fwat_i * (facw - faci) + fwat * facw_i + (T(1.0) - fwat) * faci_i;
    const T cor_i = e.RETV * esdp_i * cor * cor;
    const T dqsdtemp = fac * cor * x.qsat;
    const T dqsdtemp_i = fac_i * cor * x.qsat + fac * cor_i * x.qsat + fac * cor * y.qsat;
    // (:221-230 corqs / qlim feed only the evaporation block and are formed there)
    // :233-253
    const T crh2 = crh2_at(crh, eta_k);
    // :256-265
    T supsat, supsat_i;
    if (t < e.RTICE) {
        supsat = T(1.8) - T(0.003) * t;
        supsat_i = T(-0.003) * t_i;
    } else {
        supsat = T(1.0);
        supsat_i = T(0.0);
    }
    const T qsat = x.qsat * supsat;
    const T qsat_i = y.qsat * supsat + x.qsat * supsat_i;
    const T qcrit = crh2 * qsat;
    const T qcrit_i = crh2 * qsat_i;
    // :268-306
    const T qt = q + ql + qi;
    const T qt_i = q_i + ql_i + qi_i;
    T clc, clc_i, qc, qc_i;
    if (qt < qcrit) {
        clc = T(0.0);
        clc_i = T(0.0);
        qc = T(0.0);
        qc_i = T(0.0);
    } else if (qt >= qsat) {
        clc = T(1.0);
        clc_i = T(0.0);
        qc = (T(1.0) - scalm) * (qsat - qcrit);
        qc_i = (T(1.0) - scalm) * (qsat_i - qcrit_i);
    } else {
        const T qpd = qsat - qt;
        const T qpd_i = qsat_i - qt_i;
        const T qcd = qsat - qcrit;
        const T qcd_i = qsat_i - qcrit_i;
        const T den = qcd - scalm * (qt - qcrit);
        const T rden = frcp<T>(den);
        const T tmp1 = rsqrt_<T>(qpd * rden);
        clc = T(1.0) - tmp1;
        clc_i = T(-0.5) * frcp<T>(tmp1) * (qpd_i * den - qpd * (qcd_i - scalm * (qt_i - qcrit_i))) * rden * rden;
        if constexpr (REG) {
            const T rat = qpd * frcp<T>(qcd);
            const T yyy = rmin<T>(T(0.3), T(3.5) * rsqrt_<T>(rat * cube(T(1.0) - scalm * (T(1.0) - rat))) *
                                              frcp<T>(T(1.0) - scalm));
            clc_i *= yyy;
        }
        qc = (scalm * qpd + (T(1.0) - scalm) * qcd) * sq(clc);
        qc_i = (scalm * qpd_i + (T(1.0) - scalm) * qcd_i) * sq(clc) +
               T(2.0) * (scalm * qpd + (T(1.0) - scalm) * qcd) * clc * clc_i;
    }
    // :309-325 convective detrainment
    const T gdp = e.RG * rdp;
    const T gdp_i = -e.RG * dp_i * rdp * rdp;
    const T lude = dt * x.lude * gdp;
    const T lude_i = dt * (y.lude * gdp + x.lude * gdp_i);
    if (k < e.NLEV - 1 && lude >= e.RLMIN && x.lu1 >= e.ZEPS2) {
        const T rlu = frcp<T>(x.lu1);
        const T tmp2 = fexp<T>(xk, -lude * rlu);
        clc_i += -clc_i * (T(1.0) - tmp2) + (T(1.0) - clc) * tmp2 * (lude_i * rlu - lude * y.lu1 * rlu * rlu);
        clc += (T(1.0) - clc) * (T(1.0) - tmp2);
        qc += lude;
        qc_i += lude_i;
    }
    // :328-354 compensating subsidence
    const T rt = frcp<T>(t);
    const T fac1 = rt * kc.rRD;
    const T rho = x.ap * fac1;
    const T rho_i = (y.ap - x.ap * t_i * rt) * fac1;
    const T fac2 = frcp<T>(x.ap - e.RETV * foeew);
    const T rodqsdp = -rho * x.qsat * fac2;
    const T rodqsdp_i = (-rho_i * x.qsat - rho * y.qsat + rho * x.qsat * (y.ap - e.RETV * foeew_i) * fac2) * fac2;
    const T ldcp = fwat * lvdcp + (T(1.0) - fwat) * lsdcp;
    const T ldcp_i = fwat_i * (lvdcp - lsdcp) + fwat * lvdcp_i + (T(1.0) - fwat) * lsdcp_i;
    const T fac3 = frcp<T>(T(1.0) + ldcp * dqsdtemp);
    const T dtdzmo = e.RG * (kc.rRCPD - ldcp * rodqsdp) * fac3;
    const T dtdzmo_i = -(e.RG * (ldcp_i * rodqsdp + ldcp * rodqsdp_i) +
                         dtdzmo * (ldcp_i * dqsdtemp + ldcp * dqsdtemp_i)) * fac3;
    const T dqsdz = dqsdtemp * dtdzmo - e.RG * rodqsdp;
    const T dqsdz_i = dqsdtemp_i * dtdzmo + dqsdtemp * dtdzmo_i - e.RG * rodqsdp_i;
    // :356-373
    const T rrho = e.RD * t * rap;
    const T tmp3 = dt * dqsdz * (x.mfu + x.mfd) * rrho;
    T dqc, dqc_i;
    if (tmp3 < qc) {
        dqc = tmp3;
        dqc_i = (dt * (dqsdz_i * (x.mfu + x.mfd) + dqsdz * (y.mfu + y.mfd)) - dqc * rho_i) * rrho;
        if constexpr (REG) dqc_i *= T(0.1);
    } else {
        dqc = qc;
        dqc_i = qc_i;
    }
    qc -= dqc;
    qc_i -= dqc_i;
    // :376-386
    T qlwc = qc * fwat;
    T qlwc_i = qc_i * fwat + qc * fwat_i;
    T qiwc = qc * (T(1.0) - fwat);
    T qiwc_i = qc_i * (T(1.0) - fwat) - qc * fwat_i;
    T condl = (qlwc - ql) * kc.rdt;
    T condl_i = (qlwc_i - ql_i) * kc.rdt;
    T condi = (qiwc - qi) * kc.rdt;
    T condi_i = (qiwc_i - qi_i) * kc.rdt;
    // :390-397 maximum overlap (covpclr feeds only the evaporation block)
    if (clc > c.covptot) {
        c.covptot = clc;
        c.covptot_i = clc_i;
    }
    // :400-427 melting of incoming snow;  1/lfdcp = zden / RLMLT
    T rfln, rfln_i, sfln, sfln_i;
    if (c.sfl != T(0.0)) {
        const T ilf = zden * kc.rRLMLT;
        const T cons = kc.cons2 * dp * ilf;
        const T cons_i = kc.cons2 * (dp_i * lfdcp - dp * lfdcp_i) * ilf * ilf;
        T z2s, z2s_i;
        if (t > kc.meltp2) {
            z2s = cons * (t - kc.meltp2);
            z2s_i = cons_i * (t - kc.meltp2) + cons * t_i;
        } else {
            z2s = T(0.0);
            z2s_i = T(0.0);
        }
        T snmlt, snmlt_i;
        if (c.sfl <= z2s) {
            snmlt = c.sfl;
            snmlt_i = c.sfl_i;
        } else {
            snmlt = z2s;
            snmlt_i = z2s_i;
        }
        rfln = c.rfl + snmlt;
        rfln_i = c.rfl_i + snmlt_i;
        sfln = c.sfl - snmlt;
        sfln_i = c.sfl_i - snmlt_i;
        const T rcons = frcp<T>(cons);
        t -= snmlt * rcons;
        t_i -= (snmlt_i * cons - snmlt * cons_i) * rcons * rcons;
    } else {
        rfln = c.rfl;
        rfln_i = c.rfl_i;
        sfln = c.sfl;
        sfln_i = c.sfl_i;
    }
    // :429-503 autoconversion
    T prr = T(0.0), prr_i = T(0.0), prs = T(0.0), prs_i = T(0.0);
    if (clc > e.ZEPS2) {
        const T rclc = frcp<T>(clc);
        const T cldl = qlwc * rclc;
        const T cldl_i = qlwc_i * rclc - qlwc * clc_i * rclc * rclc;
        const T ltmp4 = fexp<T>(xk, -sq(cldl * kc.rlcrit));
        const T dl = kc.ckcodtl * (T(1.0) - ltmp4);
        const T ltmp5 = fexp<T>(xk, -dl);
        const T dl_i = (T(2.0) * (REG ? kc.ckcodtl * T(0.01) : kc.ckcodtl) * kc.rlcrit * kc.rlcrit) * ltmp4 * cldl * cldl_i;
        const T qlnew = clc * cldl * ltmp5;
        const T qlnew_i = clc_i * cldl * ltmp5 + clc * cldl_i * ltmp5 - clc * cldl * ltmp5 * dl_i;
        prr = qlwc - qlnew;
        prr_i = qlwc_i - qlnew_i;
        qlwc -= prr;
        qlwc_i -= prr_i;
        const T cldi = qiwc * rclc;
        const T cldi_i = qiwc_i * rclc - qiwc * clc_i * rclc * rclc;
        const T itmp41 = fexp<T>(xk, -sq(cldi * kc.ricrit));
        const T itmp42 = fexp<T>(xk, T(0.025) * (t - e.RTT));
        const T di = kc.ckcodti * itmp42 * (T(1.0) - itmp41);
        const T itmp5 = fexp<T>(xk, -di);
        const T di_i = (REG ? kc.ckcodti * T(0.01) : kc.ckcodti) * itmp42 *
                       (itmp41 * (T(2.0) * cldi * cldi_i * kc.ricrit * kc.ricrit - T(0.025) * t_i) + T(0.025) * t_i);
        const T qinew = clc * cldi * itmp5;
        const T qinew_i = clc_i * cldi * itmp5 + clc * cldi_i * itmp5 - clc * cldi * itmp5 * di_i;
        prs = qiwc - qinew;
        prs_i = qiwc_i - qinew_i;
        qiwc -= prs;
        qiwc_i -= prs_i;
    }
    // :506-523 new precipitation
    const T dr = kc.cons2 * dp * (prr + prs);
    const T dr_i = kc.cons2 * (dp_i * (prr + prs) + dp * (prr_i + prs_i));
    T rfreeze, rfreeze_i;
    if (t < e.RTT) {
        rfreeze = kc.cons2 * dp * prr;
        rfreeze_i = kc.cons2 * (dp_i * prr + dp * prr_i);
        sfln += dr;
        sfln_i += dr_i;
    } else {
        rfreeze = T(0.0);
        rfreeze_i = T(0.0);
        rfln += dr;
        rfln_i += dr_i;
    }
    // :526-616 precipitation evaporation (LEVAPLS2 or LDRAIN1D).  q / q_i are still the first guess of :154-156
    // here, so corqs (:221-222) and qlim (:225-230) are formed in place; covpclr is :392-397.
    T evapr = T(0.0), evapr_i = T(0.0), evaps = T(0.0), evaps_i = T(0.0);
    o.covptot = T(0.0);
    o.covptot_i = T(0.0);
    if constexpr (EVAP) {
        T covpclr = c.covptot - clc;
        T covpclr_i = c.covptot_i - clc_i;
        if (covpclr < T(0.0)) {
            covpclr = T(0.0);
            covpclr_i = T(0.0);
        }
        const T prtot = rfln + sfln;
        const T prtot_i = rfln_i + sfln_i;
        if (prtot > e.ZEPS2 && covpclr > e.ZEPS2) {
            const T corqs = T(1.0) + kc.cons3 * dqsdtemp;
            const T corqs_i = kc.cons3 * dqsdtemp_i;
            T qlim, qlim_i;
            if (q > x.qsat) {
                qlim = x.qsat;
                qlim_i = y.qsat;
            } else {
                qlim = q;
                qlim_i = q_i;
            }
            // trajectory quantities with discrete consequences (the covptot reset below, a flux that must become
            // exactly 0 when everything evaporates) use IEEE division like the reference, not x * frcp(y)
            const T rcov = frcp<T>(c.covptot);
            const T preclr = prtot * covpclr / c.covptot;
            const T preclr_i = (prtot_i * covpclr + prtot * covpclr_i) * rcov - prtot * covpclr * c.covptot_i * rcov * rcov;
            const T romc = frcp<T>(T(1.0) - clc);
            const T qe = x.qsat - (x.qsat - qlim) * covpclr * romc * romc;
            const T qe_i = y.qsat - (y.qsat * covpclr - qlim_i * covpclr + (x.qsat - qlim) * covpclr_i) * romc * romc -
                           T(2.0) * (x.qsat - qlim) * covpclr * clc_i * romc * romc * romc;
            const T tmp6 = rsqrt_<T>(x.ap * frcp<T>(c.aph_s));
            const T rcp = frcp<T>(covpclr);
            const T arg = tmp6 * preclr * rcp * T(1.0 / 0.00509);
            const T pw = rpow<T>(arg, T(0.5777));
            const T beta = e.RG * e.RPECONS * pw;
            // (0.00509 covpclr / (tmp6 preclr))^0.4223 = arg^-0.4223 = pw / arg
            const T beta_i = T(0.5777 / 0.00509) * e.RG * e.RPECONS * pw * frcp<T>(arg) *
                             ((tmp6 * preclr_i + T(0.5) * preclr * y.ap * frcp<T>(tmp6) -
                               T(0.5) * preclr * tmp6 * c.aph_s_i * frcp<T>(c.aph_s)) * rcp -
                              tmp6 * preclr * covpclr_i * rcp * rcp);
            const T rden = frcp<T>(T(1.0) + dt * beta * corqs);
            const T b = dt * beta * (x.qsat - qe) * rden;
            // the reference's dt**2 factor in the second term is kept (tangent_linear/_stencils/cloudsc2.py:565-569)
            const T b_i = dt * (beta_i * (x.qsat - qe) + beta * (y.qsat - qe_i)) * rden -
                          dt * dt * b * (beta_i * corqs + beta * corqs_i) * rden;
            const T rdtgdp = dp * frcp<T>(kc.rgdt);  // 1 / dtgdp = dp / (dt RG)
            const T dtgdp_i = -dt * e.RG * dp_i * rdp * rdp;
            T dpr = covpclr * b * rdtgdp;
            T dpr_i = (covpclr_i * b + covpclr * b_i) * rdtgdp - covpclr * b * dtgdp_i * rdtgdp * rdtgdp;
            // preclr - dpr <= 0 (:580) <=> dpr >= preclr; written as a comparison because `preclr - dpr` may be
            // contracted into an fma with the product that defines preclr, which would leave a rounding residue
            const bool all_evaporates = dpr >= preclr;
            if (dpr > preclr) {
                dpr = preclr;
                dpr_i = preclr_i;
            }
            if (all_evaporates) {
                c.covptot = clc;
                c.covptot_i = clc_i;
            }
            o.covptot = c.covptot;
            o.covptot_i = c.covptot_i;
            const T rpr = frcp<T>(prtot);
            evapr = dpr * rfln / prtot;
            evapr_i = evaporated_i<T>(dpr, dpr_i, rfln, rfln_i, prtot, prtot_i, rpr);
            rfln -= evapr;
            rfln_i -= evapr_i;
            evaps = dpr * sfln / prtot;
            evaps_i = evaporated_i<T>(dpr, dpr_i, sfln, sfln_i, prtot, prtot_i, rpr);
            sfln -= evaps;
            sfln_i -= evaps_i;
        }
    }
    // :619-659   (src = in_lude + evapr + evaps;  hh = the latent-heat weighted sum of the same three sources)
    const T src = x.lude + evapr + evaps;
    const T src_i = y.lude + evapr_i + evaps_i;
    const T hh = x.lude * ldcp + lvdcp * evapr + lsdcp * evaps;
    const T hh_i = y.lude * ldcp + x.lude * ldcp_i + lvdcp_i * evapr + lvdcp * evapr_i + lsdcp_i * evaps + lsdcp * evaps_i;
    const T dqdt = -(condl + condi) + src * gdp;
    const T dqdt_i = -(condl_i + condi_i) + src_i * gdp + src * gdp_i;
    const T tmp7 = hh - (lsdcp - lvdcp) * rfreeze;
    const T dtdt = lvdcp * condl + lsdcp * condi - tmp7 * gdp;
    const T dtdt_i = lvdcp_i * condl + lvdcp * condl_i + lsdcp_i * condi + lsdcp * condi_i -
                     (hh_i - (lsdcp_i - lvdcp_i) * rfreeze - (lsdcp - lvdcp) * rfreeze_i) * gdp - tmp7 * gdp_i;
    t += dt * dtdt;
    t_i += dt * dtdt_i;
    q += dt * dqdt;
    q_i += dt * dqdt_i;
    const T qold = q;
    const T qold_i = q_i;
    // :662 (tangent_linear/_stencils/cuadjtqs.py:55-84)
    {
        T a3, a4, a5, ad;
        if (t > e.RTT) {
            a3 = e.R3LES; a4 = e.R4LES; a5 = e.R5ALVCP; ad = e.RALVDCP;
        } else {
            a3 = e.R3IES; a4 = e.R4IES; a5 = e.R5ALSCP; ad = e.RALSDCP;
        }
        tl_cuadj_iter(e, xk, rap, y.ap, t, t_i, q, q_i, a3, a4, a5, ad);
        tl_cuadj_iter(e, xk, rap, y.ap, t, t_i, q, q_i, a3, a4, a5, ad);
    }
    // :664-673
    T dq, dq_i;
    if (qold >= q) {
        dq = qold - q;
        dq_i = qold_i - q_i;
        if constexpr (REG) dq_i *= T(0.7);
    } else {
        dq = T(0.0);
        dq_i = T(0.0);
    }
    const T dr2 = kc.cons2 * dp * dq;
    const T dr2_i = kc.cons2 * (dp_i * dq + dp * dq_i);
    // :677-703
    if (t < e.RTT) {
        rfreeze += fwat * dr2;
        rfreeze_i += fwat_i * dr2 + fwat * dr2_i;
        condi += dq * kc.rdt;
        condi_i += dq_i * kc.rdt;
        sfln += dr2;
        sfln_i += dr2_i;
    } else {
        condl += dq * kc.rdt;
        condl_i += dq_i * kc.rdt;
        rfln += dr2;
        rfln_i += dr2_i;
    }
    // :706-741
    o.clc = clc;
    o.clc_i = clc_i;
    o.tnd_q = -(condl + condi) + src * gdp;
    o.tnd_q_i = -(condl_i + condi_i) + src_i * gdp + src * gdp_i;
    const T tmp8 = hh - (lsdcp - lvdcp) * rfreeze;
    o.tnd_t = lvdcp * condl + lsdcp * condi - tmp8 * gdp;
    o.tnd_t_i = lvdcp_i * condl + lvdcp * condl_i + lsdcp_i * condi + lsdcp * condi_i -
                (hh_i - (lsdcp_i - lvdcp_i) * rfreeze - (lsdcp - lvdcp) * rfreeze_i) * gdp - tmp8 * gdp_i;
    o.tnd_ql = (qlwc - ql) * kc.rdt;
    o.tnd_ql_i = (qlwc_i - ql_i) * kc.rdt;
    o.tnd_qi = (qiwc - qi) * kc.rdt;
    o.tnd_qi_i = (qiwc_i - qi_i) * kc.rdt;
    // :744-753
    o.rfln = rfln;
    o.rfln_i = rfln_i;
    o.sfln = sfln;
    o.sfln_i = sfln_i;
    c.rfl = rfln;
    c.rfl_i = rfln_i;
    c.sfl = sfln;
    c.sfl_i = sfln_i;
    c.aph_k = x.aph1;
    c.aph_k_i = y.aph1;
    return o;
}

template <typename T, typename O>
__device__ __forceinline__ void tl_store(const MPtrs<T, NL_NUM_OUT>& out, const MPtrs<T, NL_NUM_OUT>& out_i,
                                         const Ext<T>& e, O lsb, O i, const TLOut<T>& o) {
    stg(out.p[NL_OUT_CLC], i, o.clc);
    stg(out_i.p[NL_OUT_CLC], i, o.clc_i);
    stg(out.p[NL_OUT_COVPTOT], i, o.covptot);   // :185-186 (only the evaporation block sets it non-zero)
    stg(out_i.p[NL_OUT_COVPTOT], i, o.covptot_i);
    stg(out.p[NL_OUT_TND_Q], i, o.tnd_q);
    stg(out_i.p[NL_OUT_TND_Q], i, o.tnd_q_i);
    stg(out.p[NL_OUT_TND_T], i, o.tnd_t);
    stg(out_i.p[NL_OUT_TND_T], i, o.tnd_t_i);
    stg(out.p[NL_OUT_TND_QL], i, o.tnd_ql);
    stg(out_i.p[NL_OUT_TND_QL], i, o.tnd_ql_i);
    stg(out.p[NL_OUT_TND_QI], i, o.tnd_qi);
    stg(out_i.p[NL_OUT_TND_QI], i, o.tnd_qi_i);
    // :766-774
    stg(out.p[NL_OUT_FPLSL], i + lsb, o.rfln);
    stg(out_i.p[NL_OUT_FPLSL], i + lsb, o.rfln_i);
    stg(out.p[NL_OUT_FPLSN], i + lsb, o.sfln);
    stg(out_i.p[NL_OUT_FPLSN], i + lsb, o.sfln_i);
    stg(out.p[NL_OUT_FHPSL], i + lsb, -o.rfln * e.RLVTT);
    stg(out_i.p[NL_OUT_FHPSL], i + lsb, -o.rfln_i * e.RLVTT);
    stg(out.p[NL_OUT_FHPSN], i + lsb, -o.sfln * e.RLSTT);
    stg(out_i.p[NL_OUT_FHPSN], i + lsb, -o.sfln_i * e.RLSTT);
}

// The constants of the TL level loop, pinned in VGPRs (see pin_vgpr), then the exp coefficients.
template <typename T>
__device__ __forceinline__ void pin_tl_constants(Ext<T>& e, NLK<T>& kc, ExpK<T>& xk, T& dt) {
    pin_vgprs(e.RCPD, e.RLSTT, e.RLVTT, e.RLMLT, e.R4LES, e.R4IES, e.RTT, e.R3IES, e.R3LES, e.R2ES, e.ZQMAX, e.RETV, e.R5LES,
              e.R5IES, e.RG, e.RD, kc.rdt, kc.cons2, kc.rRD, kc.rRCPD, dt);
    pin_expk(xk);
}

// :124-135, the carry at the top of a column.  Trajectory half: zero fluxes, aph[0] at byte offset `colb` and, for the
// evaporation block, the surface pressure aph[nz] at `surfb`.  Perturbation half: loaded at the column's own offsets (or at
// the zero line's, tl_masked_sweep), or formed as finc * trajectory (INC, see increment).
template <typename T, bool EVAP, typename O>
__device__ __forceinline__ TLCarry<T> tl_carry_top(const T* aph, O colb, O surfb) {
    TLCarry<T> c;
    c.rfl = c.rfl_i = c.sfl = c.sfl_i = c.covptot = c.covptot_i = T(0.0);
    c.aph_k = ldg(aph, colb);
    c.aph_s = EVAP ? ldg(aph, surfb) : T(1.0);
    return c;
}
template <typename T, bool EVAP, typename O>
__device__ __forceinline__ void tl_carry_top_i(TLCarry<T>& c, const T* aph_i, O colb, O surfb) {
    c.aph_k_i = ldg(aph_i, colb);
    c.aph_s_i = EVAP ? ldg(aph_i, surfb) : T(0.0);
}
template <typename T, bool EVAP>
__device__ __forceinline__ void tl_carry_top_inc(TLCarry<T>& c, T finc) {
    c.aph_k_i = rounded_product<T>(finc, c.aph_k);
    c.aph_s_i = EVAP ? rounded_product<T>(finc, c.aph_s) : T(0.0);
}

// INC: the perturbation fields are not read but formed as finc * in (state_increment fused in, see increment):
// 16 input streams instead of 32, no landing buffer for the second 16.
// BIG: 64-bit byte offsets (fields of 4 GiB and more, see offset_t in cloudsc2_common.hpp); instantiated without INC only.
template <typename T, bool REG, bool EVAP, bool INC = false, bool BIG = false>
__global__ void __launch_bounds__(kColBlock)
tl_kernel(Ext<T> e, NLK<T> kc, ExpK<T> xk, int nx, int nz, int64_t ls, CPtrs<T, NL_NUM_IN> in,
          CPtrs<T, NL_NUM_IN> in_i, const T* __restrict__ eta, MPtrs<T, NL_NUM_OUT> out, MPtrs<T, NL_NUM_OUT> out_i,
          T dt, T finc, int zero_supsat_i) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T* s_eta = reinterpret_cast<T*>(smem_raw);
    T* s_scalm = s_eta + (nz + 1);
    int klo, khi;
    build_level_table<T>(eta, nz, e, s_eta, s_scalm, klo, khi);
    if constexpr (sizeof(T) == 8) pin_tl_constants(e, kc, xk, dt);   // fp64 constants of the level loop -> VGPRs

    const int gcol = xcd_block() * kColBlock + threadIdx.x;
    // Lanes past the last column retire here (no workgroup barrier follows build_level_table).  They must not be carried
    // along under an `if (live)` around the stores: that branch is a merge point for hipcc's wait-count insertion, which
    // then drains every store of a level (`s_waitcnt vmcnt(0)`) before the next level's words are handed over
    // (docs/TUNING_LOG.md 3.9).
    if (gcol >= nx) return;
    using O = offset_t<BIG>;
#if CS2_TL_DIAG == 2
    const O lsb = nz < 0 ? O(ls) : O(0);   // diagnostics only (wrong results): every level reads and writes level 0 -
#else                                                  // cache-resident rows, the kernel's time without HBM
    const O lsb = O(ls) * O(sizeof(T));
#endif
    const O colb = O(gcol) * O(sizeof(T));

    const T trpaus = trpaus_prescan<T, false, O>(in.p[NL_IN_T], in.p[NL_IN_TND_CML_T], lsb, colb, dt, s_eta, klo, khi);
    const CrhCol<T> crh = crh_setup<T>(trpaus);

    // :124-135
    TLCarry<T> c = tl_carry_top<T, EVAP, O>(in.p[NL_IN_APH], colb, O(nz) * lsb + colb);
    if constexpr (INC) tl_carry_top_inc<T, EVAP>(c, finc);
    else tl_carry_top_i<T, EVAP, O>(c, in_i.p[NL_IN_APH], colb, O(nz) * lsb + colb);

    // :757-765
    stg(out.p[NL_OUT_FPLSL], colb, T(0.0));
    stg(out_i.p[NL_OUT_FPLSL], colb, T(0.0));
    stg(out.p[NL_OUT_FPLSN], colb, T(0.0));
    stg(out_i.p[NL_OUT_FPLSN], colb, T(0.0));
    stg(out.p[NL_OUT_FHPSL], colb, T(0.0));
    stg(out_i.p[NL_OUT_FHPSL], colb, T(0.0));
    stg(out.p[NL_OUT_FHPSN], colb, T(0.0));
    stg(out_i.p[NL_OUT_FHPSN], colb, T(0.0));

    O o = colb;
    if constexpr (INC) {
        LevelIn<T> xa = load_level<T, O>(in, lsb, o);
        for (int k = 0; k < nz; ++k) {
            LevelIn<T> xn = xa;
            if (k + 1 < nz) xn = load_level<T, O>(in, lsb, o + lsb);
            const LevelIn<T> ya = increment<T>(xa, finc, zero_supsat_i != 0);
            const TLOut<T> r = tl_level<T, REG, EVAP>(e, kc, xk, xa, ya, k, s_eta[k], s_scalm[k], crh, dt, c);
            tl_store<T, O>(out, out_i, e, lsb, o, r);
            drain_vmem();   // see drain_vmem
            xa = xn;
            o += lsb;
        }
    } else {
        LevelIn<T> xa = load_level<T, O>(in, lsb, o), ya = load_level<T, O>(in_i, lsb, o);
        for (int k = 0; k < nz; ++k) {
            LevelIn<T> xn = xa, yn = ya;
            if (k + 1 < nz) {
                xn = load_level<T, O>(in, lsb, o + lsb);
                yn = load_level<T, O>(in_i, lsb, o + lsb);
            }
            const TLOut<T> r = tl_level<T, REG, EVAP>(e, kc, xk, xa, ya, k, s_eta[k], s_scalm[k], crh, dt, c);
            tl_store<T, O>(out, out_i, e, lsb, o, r);
            drain_vmem();
            xa = xn;
            ya = yn;
            o += lsb;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// LDS-ring variant of the sweep.  Same prologue, same tl_level / tl_store; only the way the 32 input words of a level
// (16 trajectory + 16 perturbation fields) reach the lane differs - the load path of cloudsc2_nl.hip's nl_ring_kernel,
// restated for 32 fields:
//   * every wave owns RD slots of 32 fields x 64 columns in LDS (16 KB per slot in fp64); level k + RD - 1 is requested
//     with LDS-DMA (`global_load_lds_dwordx4`, no VGPR destination) while level k is computed.  In fp64 RD = 2 is what
//     fits a CU (4 waves x 2 x 16 KB + table): the same one level ahead as the register prefetch of tl_kernel, but
//     without its 32-double landing buffer (64 VGPRs) - the register path runs at 254-256 VGPRs + 36-96 AGPRs;
//   * one DMA instruction moves 16 B per lane = NPL columns (2 fp64 / 4 fp32): lane group g of instruction i fetches
//     field i*NPL + g of the concatenated list [in[0..15], in_i[0..15]], so field f of a slot starts at
//     f * 64 * sizeof(T) and the lane reads its own column with ds_read_b64 / _b32;
//   * the waits are counted by hand (vmcnt retires in order on gfx9): when level k is read, the operations younger than
//     its DMAs are the (RD-1) x NI DMAs of the levels in flight and the (RD-1) x 20 stores of the levels computed since.
//     Unlike nl_ring_kernel (three slots, one level of stores of slack) the count is EXACT here: with two slots a
//     stricter wait would expose the completion latency of the previous level's stores on every level.  tl_store
//     issues exactly kTLStores stores per level (20 distinct fields; tests/test_ring_isa.py counts them in the compiled ISA, and __graft_entry__.build() runs that check whenever it recompiles).
// Used when the launcher can guarantee 16-byte aligned rows and whole waves (launch_tl); every other call takes the
// register-prefetch kernel above.  Results are bit-identical (same arithmetic on the same words).
constexpr int kTLRing = 2;                  // slots per wave, fp64 and fp32
constexpr int kTLFields = 2 * NL_NUM_IN;    // input words per level and column
constexpr int kTLStores = 2 * NL_NUM_OUT;   // stores per level (tl_store)
template <typename T>
using TLRingGeom = RingGeom<T, kTLFields>;

// Wait until at most N vector-memory operations are outstanding, then read this lane's column of 16 fields of the slot
// at LDS byte address `a`.  Two statements per level (x, y): the wait and the LDS reads live in ONE asm statement with a
// memory clobber - hipcc would otherwise drain vmcnt(0) before every LDS read that follows an LDS-DMA, and no store may
// move across the wait.
template <int N, typename T>
__device__ __forceinline__ void tl_ring_read16(uint32_t a, LevelIn<T>& x) {
    if constexpr (sizeof(T) == 8)
        asm volatile("s_waitcnt vmcnt(%[n])\n\t" CS2_DS_READ16_B64 "s_waitcnt lgkmcnt(0)"
                     : CS2_LEVEL_OUTS(x)
                     : [a] "v"(a), [n] "n"(N)
                     : "memory");
    else
        asm volatile("s_waitcnt vmcnt(%[n])\n\t" CS2_DS_READ16_B32 "s_waitcnt lgkmcnt(0)"
                     : CS2_LEVEL_OUTS(x)
                     : [a] "v"(a), [n] "n"(N)
                     : "memory");
}
// eta[k] (LDS byte address ta) and scalm[k] (tb) from the level table; the table is written before the only workgroup
// barrier and never again, so no vector-memory wait is involved
__device__ __forceinline__ void tl_table_read(uint32_t ta, uint32_t tb, double& eta_k, double& scalm_k) {
    asm volatile("ds_read_b64 %0, %2\n\tds_read_b64 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(eta_k), "=&v"(scalm_k) : "v"(ta), "v"(tb) : "memory");
}
__device__ __forceinline__ void tl_table_read(uint32_t ta, uint32_t tb, float& eta_k, float& scalm_k) {
    asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(eta_k), "=&v"(scalm_k) : "v"(ta), "v"(tb) : "memory");
}

template <typename T, bool REG, bool EVAP, int RD>
__global__ void __launch_bounds__(kColBlock, 1)
tl_ring_kernel(Ext<T> e, NLK<T> kc, ExpK<T> xk, int nx, int nz, int64_t ls, CPtrs<T, NL_NUM_IN> in,
               CPtrs<T, NL_NUM_IN> in_i, const T* __restrict__ eta, MPtrs<T, NL_NUM_OUT> out, MPtrs<T, NL_NUM_OUT> out_i,
               T dt) {
    using G = TLRingGeom<T>;
    static_assert(kColBlock % 64 == 0 && RD >= 2, "whole waves, at least one level in flight");
    static_assert((RD - 1) * (G::NI + kTLStores) < 64, "vmcnt is a 6-bit counter");
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T* s_eta = reinterpret_cast<T*>(smem_raw);
    T* s_scalm = s_eta + (nz + 1);
    int klo, khi;
    build_level_table<T>(eta, nz, e, s_eta, s_scalm, klo, khi);
    if constexpr (sizeof(T) == 8) pin_tl_constants(e, kc, xk, dt);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wcol0 = xcd_block() * kColBlock + wave * 64;   // first column of this wave
    if (wcol0 >= nx) return;                                // nx % 64 == 0 (launcher): whole waves retire; the only
                                                            // workgroup barrier is inside build_level_table
    const uint32_t lsb = uint32_t(ls) * uint32_t(sizeof(T));
    const uint32_t colb = uint32_t(wcol0 + lane) * uint32_t(sizeof(T));

    const T trpaus = trpaus_prescan<T>(in.p[NL_IN_T], in.p[NL_IN_TND_CML_T], lsb, colb, dt, s_eta, klo, khi);
    const CrhCol<T> crh = crh_setup<T>(trpaus);

    // :124-135
    TLCarry<T> c = tl_carry_top<T, EVAP, uint32_t>(in.p[NL_IN_APH], colb, uint32_t(nz) * lsb + colb);
    tl_carry_top_i<T, EVAP, uint32_t>(c, in_i.p[NL_IN_APH], colb, uint32_t(nz) * lsb + colb);
    // :757-765
    stg(out.p[NL_OUT_FPLSL], colb, T(0.0));
    stg(out_i.p[NL_OUT_FPLSL], colb, T(0.0));
    stg(out.p[NL_OUT_FPLSN], colb, T(0.0));
    stg(out_i.p[NL_OUT_FPLSN], colb, T(0.0));
    stg(out.p[NL_OUT_FHPSL], colb, T(0.0));
    stg(out_i.p[NL_OUT_FHPSL], colb, T(0.0));
    stg(out.p[NL_OUT_FHPSN], colb, T(0.0));
    stg(out_i.p[NL_OUT_FHPSN], colb, T(0.0));
    // consume the prologue's ordinary loads BEFORE the first DMA is issued: hipcc drains vmcnt(0) at the first use of
    // an ordinary load's result while an LDS-DMA is in flight, which would empty the ring inside level 0
    pin_vgpr(c.aph_k);
    pin_vgpr(c.aph_k_i);
    if constexpr (EVAP) { pin_vgpr(c.aph_s); pin_vgpr(c.aph_s_i); }
    { T tp = crh.rh2; pin_vgpr(tp); }

    // per-lane DMA sources: lane group g of instruction i walks field i*NPL + g of [in | in_i], NPL adjacent columns
    // per lane; aph and lu are read one half level below (aph[k+1], lu[k+1]: :171, :311)
    constexpr int LPG = 64 / G::NPL;   // lanes per group
    const int g = lane / LPG, l = lane % LPG;
    const char* src[G::NI];
#pragma unroll
    for (int i = 0; i < G::NI; ++i) {
        const int f0 = i * G::NPL;                       // first field of this instruction (compile-time)
        const T* base = f0 < NL_NUM_IN ? in.p[f0] : in_i.p[f0 - NL_NUM_IN];
        int f = f0;
#pragma unroll
        for (int j = 1; j < G::NPL; ++j)
            if (g == j) {
                base = (f0 + j) < NL_NUM_IN ? in.p[f0 + j] : in_i.p[f0 + j - NL_NUM_IN];
                f = f0 + j;
            }
        const int fn = f % NL_NUM_IN;
        const uint32_t lev1 = (fn == NL_IN_APH || fn == NL_IN_LU) ? lsb : 0u;
        src[i] = reinterpret_cast<const char*>(base) + (uint32_t(wcol0 + G::NPL * l) * uint32_t(sizeof(T)) + lev1);
    }
    // LDS: [eta | scalm table][pad][wave 0: RD slots][wave 1: RD slots] ...
    const uint32_t tab_bytes = (2u * uint32_t(nz + 1) * uint32_t(sizeof(T)) + 1023u) & ~1023u;
    const uint32_t ring0 = tab_bytes + uint32_t(wave) * uint32_t(RD * G::SLOT);
    auto issue = [&](int slot) {
#pragma unroll
        for (int i = 0; i < G::NI; ++i) {
            __builtin_amdgcn_global_load_lds((glb_void_ptr)src[i],
                                             (lds_void_ptr)(&smem_raw[ring0 + uint32_t(slot * G::SLOT + i * 1024)]), 16, 0,
                                             kDmaNT);
            src[i] += lsb;
        }
    };
#pragma unroll
    for (int j = 0; j < RD - 1; ++j)
        if (j < nz) issue(j);

    // operations younger than level k's DMAs when level k is read: see the header of this kernel
    constexpr int NFULL = (RD - 1) * (G::NI + kTLStores);
    constexpr int NHEAD = (RD - 1) * G::NI;   // the first RD-1 levels: no stores counted (stricter = safe)
    const uint32_t rd_lane = ring0 + uint32_t(lane) * uint32_t(sizeof(T));
    const uint32_t tb_off = uint32_t(nz + 1) * uint32_t(sizeof(T));
    constexpr uint32_t YOFF = uint32_t(NL_NUM_IN) * 64u * uint32_t(sizeof(T));   // the perturbation half of a slot
    uint32_t o = colb;
    int slot = 0, pslot = RD - 1;
    for (int k = 0; k < nz; ++k) {
        const bool more = k + RD - 1 < nz;
        if (more) issue(pslot);
        LevelIn<T> x, y;
        T eta_k, scalm_k;
        const uint32_t a = rd_lane + uint32_t(slot * G::SLOT);
        const uint32_t ta = uint32_t(k) * uint32_t(sizeof(T));
        if (!more) tl_ring_read16<0>(a, x);   // tail: drain
        else if (k < RD - 1) tl_ring_read16<NHEAD>(a, x);
        else tl_ring_read16<NFULL>(a, x);
        tl_ring_read16<63>(a + YOFF, y);      // same level, already covered by the wait above (63 = no further wait)
        tl_table_read(ta, ta + tb_off, eta_k, scalm_k);
        const TLOut<T> r = tl_level<T, REG, EVAP>(e, kc, xk, x, y, k, eta_k, scalm_k, crh, dt, c);
        tl_store<T, uint32_t>(out, out_i, e, lsb, o, r);
        o += lsb;
        slot = slot + 1 == RD ? 0 : slot + 1;
        pslot = pslot + 1 == RD ? 0 : pslot + 1;
    }
}

template <typename T>
int launch_tl(const Cloudsc2Params& p, int nx, int nz, int64_t ls, const T* const* in, const T* const* in_i,
              const T* eta, T* const* out, T* const* out_i, double dt, hipStream_t stream, double inc_f) {
    // in_i == nullptr: the fused state_increment variant - perturbations formed in the kernel as T(inc_f) * in
    const bool inc = in_i == nullptr;
    const T tinc = static_cast<T>(inc_f);
    const int zsi = p.IGNORE_SUPSAT ? 1 : 0;
    const bool evap = evap_on(p);
    const Ext<T> e = make_ext<T>(p);
    const auto ci = pack_ptrs<CPtrs<T, NL_NUM_IN>>(in), cii = pack_ptrs<CPtrs<T, NL_NUM_IN>>(in_i);
    const auto co = pack_ptrs<MPtrs<T, NL_NUM_OUT>>(out), coi = pack_ptrs<MPtrs<T, NL_NUM_OUT>>(out_i);
    const dim3 grid((nx + kColBlock - 1) / kColBlock);
    const size_t smem = 2 * size_t(nz + 1) * sizeof(T);
    const T tdt = static_cast<T>(dt);
    const NLK<T> kc = make_nlk<T>(p, dt, evap);
    const ExpK<T> xk = make_expk<T>();
    // fields of 4 GiB and more: the register-path kernel with 64-bit offsets (not the fused-increment variant)
    const bool big = !fits_u32_offsets<T>(nz, ls);
    if (big && inc) return -2;
    // LDS-ring variant: whole waves, 16-byte aligned rows of every input field (the DMA moves 16 B per lane)
    bool ring = !big && !inc && nx % 64 == 0 && nz >= kTLRing && (ls * int64_t(sizeof(T))) % 16 == 0;
    for (int i = 0; i < NL_NUM_IN && ring; ++i)
        ring = reinterpret_cast<uintptr_t>(in[i]) % 16 == 0 && reinterpret_cast<uintptr_t>(in_i[i]) % 16 == 0;
    const size_t rsmem = ring_lds_bytes<TLRingGeom<T>, T>(nz, kTLRing);
    ring = ring && rsmem <= kLdsPerCU;   // very tall columns take the register path
    int dev = 0;
    if (ring)
        if (const int rc = current_device(dev)) return rc;
    if (ring && sizeof(T) == 8) {
        // fp64 (two slots per wave = the register path's one level ahead): the ring wins wherever part of the chip is
        // latency-bound - 8 192 .. 49 152 columns -3.5 .. -6 %, 98 304 (1.5 workgroups per CU) -3.7 % - and loses
        // 1.5-2 % when every CU holds the same number of workgroups for the whole launch and HBM is saturated
        // (65 536: 720 vs 710 us, 131 072: 1 518 vs 1 488 us; profiles/r02/ab_tl_ring.txt).  Rule: register path when
        // at least 3/4 of the launch's workgroup rounds are full.  fp32 (8 KB slots): the ring wins at every size
        // measured (65 536: 337 vs 389 us; 524 288: 2 986 vs 3 049 us).
        const int64_t c = device_cus(dev), gx = grid.x;
        const int64_t full = gx / c, rounds = (gx + c - 1) / c;
        ring = 4 * full < 3 * rounds;
    }
    // The ring always needs the opt-in, which launch_tail makes above kLdsOptIn: its kColBlock / 64 = 4 waves x kTLRing = 2
    // slots of 32 fields x 64 columns are 4 x 2 x 8 KiB = 64 KiB in fp32 and 4 x 2 x 16 KiB = 128 KiB in fp64, and the
    // level table in front of them is at least 1 KiB (ring_lds_bytes rounds it up).
    if (ring)
        return with_flags(
            [&](auto REG, auto EVAP) {
                return launch_tail<tl_ring_kernel<T, REG, EVAP, kTLRing>>({grid, rsmem, stream, "cs2::tl_ring_kernel", false, dev}, e,
                                                                          kc, xk, nx, nz, ls, ci, cii, eta, co, coi, tdt);
            },
            p.LREGCL != 0, evap);
    const Launch l{grid, smem, stream, big ? "cs2::tl_kernel<big>" : inc ? "cs2::tl_kernel<inc>" : "cs2::tl_kernel"};
    return with_flags(
        [&](auto REG, auto EVAP, auto INC, auto BIG) {
            if constexpr (INC && BIG) return -2;   // refused above: no such instantiation
            else return launch_tail<tl_kernel<T, REG, EVAP, INC, BIG>>(l, e, kc, xk, nx, nz, ls, ci, cii, eta, co, coi, tdt, tinc, zsi);
        },
        p.LREGCL != 0, evap, inc, big);
}

template int launch_tl<double>(const Cloudsc2Params&, int, int, int64_t, const double* const*, const double* const*,
                               const double*, double* const*, double* const*, double, hipStream_t, double);
template int launch_tl<float>(const Cloudsc2Params&, int, int, int64_t, const float* const*, const float* const*,
                              const float*, float* const*, float* const*, double, hipStream_t, double);

// ------------------------------------------------------------------------------------------------------------------
// Masked tangent-linear (BUILD EXTENSION, C ABI cloudsc2_tl_masked_*): the Jacobian-vector product as an
// automatic-differentiation framework asks for it - perturbations on a few inputs, a few perturbed outputs, the NL outputs
// only on request.  The register-path sweep of tl_kernel (same tl_level, one level of prefetch, stores drained per level)
// with the mechanism of ad_masked_kernel (cloudsc2_ad.hip): every load is issued, an absent perturbation reads this lane's
// word of the caller's zero line (the launcher has put the line in place of the field's pointer; one v_cndmask on a
// wave-uniform bit of `have` picks the offset), an unwanted output is skipped by a wave-uniform branch around its store.
// The field pointers are read from the kernarg segment (KernArgs): 52 of them do not fit the SGPRs beside the constants.
template <typename T>
struct TLMaskedArgs {
    Ext<T> e;
    NLK<T> kc;
    ExpK<T> xk;
    int nx, nz;
    int64_t ls;
    CPtrs<T, NL_NUM_IN> in;
    CPtrs<T, NL_NUM_IN> in_i;     // an absent perturbation: the zero line
    const T* eta;
    MPtrs<T, NL_NUM_OUT> out;     // all or none (kTLWantNL)
    MPtrs<T, NL_NUM_OUT> out_i;   // an unwanted field: nullptr, never used (its bit of `want` is 0)
    T dt;
    uint32_t have;                // bit f: perturbation f (NL_IN_*) is a field of the call
    uint32_t want;                // bit f: out_i[f] (NL_OUT_*) is written; kTLWantNL: the ten NL outputs are
};
constexpr uint32_t kTLWantNL = 1u << 31;
template <typename T>
struct TLMaskedFields : KernArgs<TLMaskedArgs<T>> {
    __device__ __forceinline__ const T* in(int i) const { return this->ka->in.p[i]; }
    __device__ __forceinline__ const T* in_i(int i) const { return this->ka->in_i.p[i]; }
    __device__ __forceinline__ T* out(int i) const { return this->ka->out.p[i]; }
    __device__ __forceinline__ T* out_i(int i) const { return this->ka->out_i.p[i]; }
};
// The same call for every MEMBER of an ensemble (tl_ens_kernel / tl_ens_step_kernel, C ABI cloudsc2_tl_ens_* /
// cloudsc2_tl_step_ens_*): see ens_block.  TLEnsFields is TLMaskedFields moved to one member: the member's base `mb`
// (elements; wave-uniform) is added to the field pointer as a 64-bit scalar, the way tl_dirs_sweep adds the direction base;
// an absent perturbation keeps the zero line's pointer (the line is 512 bytes long).  An unwanted output's pointer is never used.
template <typename T, typename G = EnsGeom>
struct TLEnsArgs {
    TLMaskedArgs<T> m;            // at kernarg offset 0
    G g;                          // EnssGeom: the shared-state form (tl_enss_kernel / tl_enss_step_kernel)
};
template <typename T>
struct TLEnsFields : KernArgs<TLEnsArgs<T>> {
    int64_t mb;
    uint32_t have;
    __device__ __forceinline__ const T* in(int i) const { return this->ka->m.in.p[i] + mb; }
    __device__ __forceinline__ const T* in_i(int i) const { return this->ka->m.in_i.p[i] + ((have >> i & 1u) ? mb : int64_t(0)); }
    __device__ __forceinline__ T* out(int i) const { return this->ka->m.out.p[i] + mb; }
    __device__ __forceinline__ T* out_i(int i) const { return this->ka->m.out_i.p[i] + mb; }
};
// TLEnsFields whose SHARED state inputs (bit i of `sh`, EnssGeom::shared) keep the call's pointer: the base is selected the
// way `in_i` selects the zero line's.  Perturbations and outputs stay per member.
template <typename T>
struct TLEnssFields : TLEnsFields<T> {
    uint32_t sh;
    __device__ __forceinline__ const T* in(int i) const {
        return this->ka->m.in.p[i] + ((sh >> i & 1u) ? int64_t(0) : this->mb);
    }
};

// load_level with a per-field offset: the field's own, or `zo` into the zero line.  SKIPQ: the qsat word is not read (the
// step kernels form it from the level's t and ap words)
template <typename T, bool SKIPQ = false, typename P>
__device__ __forceinline__ LevelIn<T> load_level_masked(const P& ptr, uint32_t have, uint32_t lsb, uint32_t o, uint32_t zo) {
    const auto at = [&](int f, uint32_t x) { return (have >> f & 1u) ? x : zo; };
    LevelIn<T> x;
    x.ap = ldg(ptr(NL_IN_AP), at(NL_IN_AP, o));
    x.aph1 = ldg(ptr(NL_IN_APH), at(NL_IN_APH, o + lsb));
    x.lu1 = ldg(ptr(NL_IN_LU), at(NL_IN_LU, o + lsb));
    x.lude = ldg(ptr(NL_IN_LUDE), at(NL_IN_LUDE, o));
    x.mfd = ldg(ptr(NL_IN_MFD), at(NL_IN_MFD, o));
    x.mfu = ldg(ptr(NL_IN_MFU), at(NL_IN_MFU, o));
    x.q = ldg(ptr(NL_IN_Q), at(NL_IN_Q, o));
    x.qi = ldg(ptr(NL_IN_QI), at(NL_IN_QI, o));
    x.ql = ldg(ptr(NL_IN_QL), at(NL_IN_QL, o));
    if constexpr (SKIPQ) x.qsat = T(0.0);
    else x.qsat = ldg(ptr(NL_IN_QSAT), at(NL_IN_QSAT, o));
    x.supsat = ldg(ptr(NL_IN_SUPSAT), at(NL_IN_SUPSAT, o));
    x.t = ldg(ptr(NL_IN_T), at(NL_IN_T, o));
    x.tq = ldg(ptr(NL_IN_TND_CML_Q), at(NL_IN_TND_CML_Q, o));
    x.tqi = ldg(ptr(NL_IN_TND_CML_QI), at(NL_IN_TND_CML_QI, o));
    x.tql = ldg(ptr(NL_IN_TND_CML_QL), at(NL_IN_TND_CML_QL, o));
    x.tt = ldg(ptr(NL_IN_TND_CML_T), at(NL_IN_TND_CML_T, o));
    return x;
}

// tl_store, each field under its bit of `want`
template <typename T, typename FP>
__device__ __forceinline__ void tl_store_masked(const FP& F, uint32_t want, const Ext<T>& e, uint32_t lsb, uint32_t i,
                                                const TLOut<T>& o) {
#define CS2_WANT(f) (want >> (f) & 1u)
    if (want & kTLWantNL) {
        stg(F.out(NL_OUT_CLC), i, o.clc);
        stg(F.out(NL_OUT_COVPTOT), i, o.covptot);
        stg(F.out(NL_OUT_TND_Q), i, o.tnd_q);
        stg(F.out(NL_OUT_TND_T), i, o.tnd_t);
        stg(F.out(NL_OUT_TND_QL), i, o.tnd_ql);
        stg(F.out(NL_OUT_TND_QI), i, o.tnd_qi);
        stg(F.out(NL_OUT_FPLSL), i + lsb, o.rfln);
        stg(F.out(NL_OUT_FPLSN), i + lsb, o.sfln);
        stg(F.out(NL_OUT_FHPSL), i + lsb, -o.rfln * e.RLVTT);
        stg(F.out(NL_OUT_FHPSN), i + lsb, -o.sfln * e.RLSTT);
    }
    if (CS2_WANT(NL_OUT_CLC)) stg(F.out_i(NL_OUT_CLC), i, o.clc_i);
    if (CS2_WANT(NL_OUT_COVPTOT)) stg(F.out_i(NL_OUT_COVPTOT), i, o.covptot_i);
    if (CS2_WANT(NL_OUT_TND_Q)) stg(F.out_i(NL_OUT_TND_Q), i, o.tnd_q_i);
    if (CS2_WANT(NL_OUT_TND_T)) stg(F.out_i(NL_OUT_TND_T), i, o.tnd_t_i);
    if (CS2_WANT(NL_OUT_TND_QL)) stg(F.out_i(NL_OUT_TND_QL), i, o.tnd_ql_i);
    if (CS2_WANT(NL_OUT_TND_QI)) stg(F.out_i(NL_OUT_TND_QI), i, o.tnd_qi_i);
    if (CS2_WANT(NL_OUT_FPLSL)) stg(F.out_i(NL_OUT_FPLSL), i + lsb, o.rfln_i);
    if (CS2_WANT(NL_OUT_FPLSN)) stg(F.out_i(NL_OUT_FPLSN), i + lsb, o.sfln_i);
    if (CS2_WANT(NL_OUT_FHPSL)) stg(F.out_i(NL_OUT_FHPSL), i + lsb, -o.rfln_i * e.RLVTT);
    if (CS2_WANT(NL_OUT_FHPSN)) stg(F.out_i(NL_OUT_FHPSN), i + lsb, -o.sfln_i * e.RLSTT);
#undef CS2_WANT
}
// :757-765: zeros on the top flux half-level, under the same bits
template <typename T, typename FP, typename O>
__device__ __forceinline__ void tl_zero_top_flux(const FP& F, uint32_t want, O colb) {
    if (want & kTLWantNL) {
        stg(F.out(NL_OUT_FPLSL), colb, T(0.0));
        stg(F.out(NL_OUT_FPLSN), colb, T(0.0));
        stg(F.out(NL_OUT_FHPSL), colb, T(0.0));
        stg(F.out(NL_OUT_FHPSN), colb, T(0.0));
    }
    if (want >> NL_OUT_FPLSL & 1u) stg(F.out_i(NL_OUT_FPLSL), colb, T(0.0));
    if (want >> NL_OUT_FPLSN & 1u) stg(F.out_i(NL_OUT_FPLSN), colb, T(0.0));
    if (want >> NL_OUT_FHPSL & 1u) stg(F.out_i(NL_OUT_FHPSL), colb, T(0.0));
    if (want >> NL_OUT_FHPSN & 1u) stg(F.out_i(NL_OUT_FHPSN), colb, T(0.0));
}

// The sweep of tl_masked_kernel and of tl_step_kernel (one copy).  STEP: `saturation` and its tangent-linear are fused in
// (C ABI cloudsc2_tl_step_*): in_qsat and its perturbation are not read; the level's qsat is saturation_point_d's value of
// the level's t and ap words (LPHYLIN form, what cloudsc2_nl_fused_* computes) and the perturbation the level function
// sees is g_t * t_i + g_ap * ap_i - formed at the head of the level's arithmetic, behind the prefetch of the next level.
// ENS: one member of an ensemble per workgroup (`g`: EnsGeom; the field pointers are TLEnsFields').
// G = EnssGeom: the members share part of their state and may each have an `eta` (C ABI cloudsc2_tl_enss_* /
// cloudsc2_tl_step_enss_*; see EnssGeom): the member is decoded in front of the level table, which is built from the member's
// own level vector; the field pointers are TLEnssFields'.
template <typename T, bool REG, bool EVAP, bool STEP, bool ENS = false, typename G = EnsGeom>
__device__ __forceinline__ void tl_masked_sweep(const TLMaskedArgs<T>& A, const G g = G{}) {
    constexpr bool SH = kSharedGeom<G>;
    static_assert(ENS || !SH, "shared state is an ensemble form");
    Ext<T> e = A.e;
    NLK<T> kc = A.kc;
    ExpK<T> xk = A.xk;
    const int nx = A.nx, nz = A.nz;
    const int64_t ls = A.ls;
    const T* __restrict__ eta = A.eta;
    T dt = A.dt;
    const uint32_t have = A.have, want = A.want;
    typename std::conditional<SH, TLEnssFields<T>, typename std::conditional<ENS, TLEnsFields<T>, TLMaskedFields<T>>::type>::type F;
    const auto F_in = [&](int i) { return F.in(i); };
    const auto F_in_i = [&](int i) { return F.in_i(i); };
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T* s_eta = reinterpret_cast<T*>(smem_raw);
    T* s_scalm = s_eta + (nz + 1);
    int klo, khi;
    int member = 0, cblock = 0;
    if constexpr (SH) {
        cblock = enss_block(g, member);
        eta += member * g.eta_ms;
    }
    build_level_table<T>(eta, nz, e, s_eta, s_scalm, klo, khi);
    if constexpr (sizeof(T) == 8) pin_tl_constants(e, kc, xk, dt);

    int gcol;
    if constexpr (ENS) {
        if constexpr (!SH) cblock = ens_block(g.bpm, member);
        gcol = cblock * kColBlock + threadIdx.x;
        F.mb = member * g.ms;
        F.have = have;
        if constexpr (SH) F.sh = g.shared;
    } else {
        gcol = xcd_block() * kColBlock + threadIdx.x;
    }
    if (gcol >= nx) return;   // see tl_kernel
    using O = uint32_t;
    const O lsb = O(ls) * O(sizeof(T));
    const O colb = O(gcol) * O(sizeof(T));
    const O zo = O(threadIdx.x & (kWave - 1)) * O(sizeof(T));   // this lane's word of the zero line
    const auto at_aph = [&](O x) { return (have >> NL_IN_APH & 1u) ? x : zo; };

    const T trpaus = trpaus_prescan<T, false, O>(F.in(NL_IN_T), F.in(NL_IN_TND_CML_T), lsb, colb, dt, s_eta, klo, khi);
    const CrhCol<T> crh = crh_setup<T>(trpaus);

    // :124-135
    TLCarry<T> c = tl_carry_top<T, EVAP, O>(F.in(NL_IN_APH), colb, O(nz) * lsb + colb);
    tl_carry_top_i<T, EVAP, O>(c, F.in_i(NL_IN_APH), at_aph(colb), at_aph(O(nz) * lsb + colb));
    tl_zero_top_flux<T>(F, want, colb);   // :757-765

    O o = colb;
    LevelIn<T> xa = load_level<T, O>(F_in, lsb, o, STEP), ya = load_level_masked<T, STEP>(F_in_i, have, lsb, o, zo);
    for (int k = 0; k < nz; ++k) {
        F.fresh();
        LevelIn<T> xn = xa, yn = ya;
        if (k + 1 < nz) {
            xn = load_level<T, O>(F_in, lsb, o + lsb, STEP);
            yn = load_level_masked<T, STEP>(F_in_i, have, lsb, o + lsb, zo);
        }
        if constexpr (STEP) {
            const SatD<T> s = saturation_point_d<T, 0>(e, xk, xa.t, xa.ap);
            xa.qsat = s.qsat;
            ya.qsat = s.g_t * ya.t + s.g_ap * ya.ap;
        }
        const TLOut<T> r = tl_level<T, REG, EVAP>(e, kc, xk, xa, ya, k, s_eta[k], s_scalm[k], crh, dt, c);
        tl_store_masked<T>(F, want, e, lsb, o, r);
        drain_vmem();   // see drain_vmem
        xa = xn;
        ya = yn;
        o += lsb;
    }
}

template <typename T, bool REG, bool EVAP>
__global__ void __launch_bounds__(kColBlock)
tl_masked_kernel(const TLMaskedArgs<T> A) {
    tl_masked_sweep<T, REG, EVAP, false>(A);
}

// `saturation` + cloudsc2_tl_masked in one launch (BUILD EXTENSION, C ABI cloudsc2_tl_step_*): see tl_masked_sweep
template <typename T, bool REG, bool EVAP>
__global__ void __launch_bounds__(kColBlock)
tl_step_kernel(const TLMaskedArgs<T> A) {
    tl_masked_sweep<T, REG, EVAP, true>(A);
}

// tl_masked_kernel / tl_step_kernel for the members of an ensemble, one launch (BUILD EXTENSION, C ABI cloudsc2_tl_ens_* /
// cloudsc2_tl_step_ens_*): see TLEnsArgs
template <typename T, bool REG, bool EVAP>
__global__ void __launch_bounds__(kColBlock)
tl_ens_kernel(const TLEnsArgs<T> A) {
    tl_masked_sweep<T, REG, EVAP, false, true>(A.m, A.g);
}

template <typename T, bool REG, bool EVAP>
__global__ void __launch_bounds__(kColBlock)
tl_ens_step_kernel(const TLEnsArgs<T> A) {
    tl_masked_sweep<T, REG, EVAP, true, true>(A.m, A.g);
}

// tl_ens_kernel / tl_ens_step_kernel for members that share part of their state (BUILD EXTENSION, C ABI cloudsc2_tl_enss_* /
// cloudsc2_tl_step_enss_*): see EnssGeom
template <typename T, bool REG, bool EVAP>
__global__ void __launch_bounds__(kColBlock)
tl_enss_kernel(const TLEnsArgs<T, EnssGeom> A) {
    tl_masked_sweep<T, REG, EVAP, false, true, EnssGeom>(A.m, A.g);
}

template <typename T, bool REG, bool EVAP>
__global__ void __launch_bounds__(kColBlock)
tl_enss_step_kernel(const TLEnsArgs<T, EnssGeom> A) {
    tl_masked_sweep<T, REG, EVAP, true, true, EnssGeom>(A.m, A.g);
}

// The arguments of a masked tangent-linear call as the kernels take them (launch_tl_masked; launch_tl_dirs for direction 0):
// in_i[f] == nullptr: perturbation f is zero everywhere (read from `zero`) and not in `have`; out == nullptr: no NL outputs;
// out_i[f] == nullptr: not in `want`, not written.
template <typename T>
static TLMaskedArgs<T> fill_tl_masked_args(const TLCall<T>& c) {
    TLMaskedArgs<T> args;
    args.e = make_ext<T>(*c.p);
    args.kc = make_nlk<T>(*c.p, c.dt, evap_on(*c.p));
    args.xk = make_expk<T>();
    args.nx = c.nx; args.nz = c.nz; args.ls = c.ls;
    args.have = 0;
    args.want = c.out ? kTLWantNL : 0u;
    args.in = pack_ptrs<CPtrs<T, NL_NUM_IN>>(c.in);
    args.out = pack_ptrs<MPtrs<T, NL_NUM_OUT>>(c.out);
    args.out_i = pack_ptrs<MPtrs<T, NL_NUM_OUT>>(c.out_i);
    for (int i = 0; i < NL_NUM_IN; ++i) {
        args.in_i.p[i] = c.in_i[i] ? c.in_i[i] : c.zero;
        if (c.in_i[i]) args.have |= 1u << i;
    }
    for (int i = 0; i < NL_NUM_OUT; ++i)
        if (c.out_i[i]) args.want |= 1u << i;
    args.eta = c.eta;
    args.dt = static_cast<T>(c.dt);
    return args;
}

// Always the register path; 32-bit offsets only.  kStep: tl_step_kernel (in[NL_IN_QSAT] and in_i[NL_IN_QSAT] are not read).
// kEns: the ensemble form (tl_ens_kernel / tl_ens_step_kernel) - every field pointer is member 0's, member m lies
// m * ms elements behind it; the caller has checked nmem and ms.  kShared (with kEns): tl_enss_kernel / tl_enss_step_kernel -
// the geometry is enss_geom's.
template <typename T>
int launch_tl_masked(const TLCall<T>& c) {
    if (!fits_u32_offsets<T>(c.nz, c.ls)) return -2;
    const bool step = c.is(kStep);
    const int nmem = c.is(kEns) ? c.members.nmem : 0;
    if (c.is(kShared) && nmem < 1) return -1;
    TLEnsArgs<T> ens;
    const TLMaskedArgs<T>& args = ens.m = fill_tl_masked_args<T>(c);
    const int bpm = (c.nx + kColBlock - 1) / kColBlock;
    const dim3 grid(bpm);
    const size_t smem = 2 * size_t(c.nz + 1) * sizeof(T);
    if (nmem > 0 && int64_t(nmem) * bpm > kMaxGrid) return -2;
    ens.g.ms = c.members.ms; ens.g.bpm = bpm;
    const dim3 egrid(unsigned(nmem > 0 ? nmem : 1) * unsigned(bpm));
    return with_flags(
        [&](auto REG, auto EVAP, auto STEP, auto ENS, auto SH) {
            if constexpr (ENS && SH) {
                constexpr auto kern = STEP ? tl_enss_step_kernel<T, REG, EVAP> : tl_enss_kernel<T, REG, EVAP>;
                const TLEnsArgs<T, EnssGeom> enss = {args, enss_geom(c.members, bpm)};
                return launch_tail<kern>({egrid, smem, c.stream, step ? "cs2::tl_enss_step_kernel" : "cs2::tl_enss_kernel"}, enss);
            } else if constexpr (ENS) {
                constexpr auto kern = STEP ? tl_ens_step_kernel<T, REG, EVAP> : tl_ens_kernel<T, REG, EVAP>;
                return launch_tail<kern>({egrid, smem, c.stream, step ? "cs2::tl_ens_step_kernel" : "cs2::tl_ens_kernel"}, ens);
            } else {
                constexpr auto kern = STEP ? tl_step_kernel<T, REG, EVAP> : tl_masked_kernel<T, REG, EVAP>;
                return launch_tail<kern>({grid, smem, c.stream, step ? "cs2::tl_step_kernel" : "cs2::tl_masked_kernel"}, args);
            }
        },
        c.p->LREGCL != 0, evap_on(*c.p), step, nmem > 0, c.is(kShared));
}

template int launch_tl_masked<double>(const TLCall<double>&);
template int launch_tl_masked<float>(const TLCall<float>&);

// ------------------------------------------------------------------------------------------------------------------
// Masked tangent-linear over `ndir` DIRECTIONS on one trajectory (BUILD EXTENSION, C ABI cloudsc2_tl_multi_* /
// cloudsc2_tl_multi_step_*): a Jacobian block, an ensemble of perturbations pushed through one linearisation.  Direction d
// of a present perturbation lies d * in_ds elements behind direction 0, direction d of a wanted output d * out_ds elements.
// Per column the pre-scan, the level table and the first `aph` words are formed once; per level the 16 (STEP: 15) state
// words are loaded once (next level prefetched, as in tl_masked_sweep), saturation_point_d runs once, the NL outputs are
// stored once.  Inside the level a RUNTIME loop over the directions loads one direction's perturbation words ahead (the
// next direction of this level, or direction 0 of the next level), calls the unchanged tl_level and stores under `want`.
//   * tl_level advances the whole carry.  Its nonlinear half is the same for every direction: it is snapshot in front of the
//     direction loop and every direction starts from the snapshot, so it advances exactly once per level.
//   * the `_i` half of the carry (five words per direction) lives in LDS slots [word][d][threadIdx.x] that no other lane
//     touches: no barrier.  kTLMaxDirs * 5 * 256 words = 80 KB in fp64 (one workgroup per CU at these kernels' one wave per
//     SIMD), 40 KB in fp32; the launcher sizes the slots by the call's ndir and opts in beyond 64 KB.
//   * the direction base is wave-uniform: it is added to the field pointer as a 64-bit scalar (an absent field keeps the
//     zero line's pointer), the per-lane offsets stay 32-bit.  Every load is issued; at the last direction of the last level
//     the look-ahead re-reads direction 0 of that level.
constexpr int kTLMaxDirs = CLOUDSC2_TL_MAX_DIRS;
constexpr int kTLCarryWords = 5;   // rfl_i, sfl_i, covptot_i, aph_k_i, aph_s_i
template <typename T>
struct TLDirsArgs {
    TLMaskedArgs<T> m;             // at kernarg offset 0: TLMaskedFields reads the pointers from there
    int64_t in_ds, out_ds;         // direction strides, in elements
    int ndir;
};
// TLMaskedFields with the output perturbations moved to one direction (what tl_store_masked is handed)
template <typename T>
struct TLDirFields {
    const TLMaskedFields<T>& F;
    int64_t ob;
    __device__ __forceinline__ T* out(int i) const { return F.out(i); }
    __device__ __forceinline__ T* out_i(int i) const { return F.out_i(i) + ob; }
};

template <typename T>
inline size_t tl_dirs_lds_bytes(int nz, int ndir) {
    return (2 * size_t(nz + 1) + size_t(kTLCarryWords) * ndir * kColBlock) * sizeof(T);
}

template <typename T, bool REG, bool EVAP, bool STEP>
__device__ __forceinline__ void tl_dirs_sweep(const TLDirsArgs<T>& A) {
    Ext<T> e = A.m.e;
    NLK<T> kc = A.m.kc;
    ExpK<T> xk = A.m.xk;
    const int nx = A.m.nx, nz = A.m.nz, ndir = A.ndir;
    const int64_t ls = A.m.ls, in_ds = A.in_ds, out_ds = A.out_ds;
    const T* __restrict__ eta = A.m.eta;
    T dt = A.m.dt;
    const uint32_t have = A.m.have, want = A.m.want;
    TLMaskedFields<T> F;
    const auto F_in = [&](int i) { return F.in(i); };
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T* s_eta = reinterpret_cast<T*>(smem_raw);
    T* s_scalm = s_eta + (nz + 1);
    T* s_carry = s_scalm + (nz + 1) + threadIdx.x;   // word w of direction d: s_carry[(w * ndir + d) * kColBlock]
    int klo, khi;
    build_level_table<T>(eta, nz, e, s_eta, s_scalm, klo, khi);
    if constexpr (sizeof(T) == 8) pin_tl_constants(e, kc, xk, dt);

    const int gcol = xcd_block() * kColBlock + threadIdx.x;
    if (gcol >= nx) return;   // see tl_kernel
    using O = uint32_t;
    const O lsb = O(ls) * O(sizeof(T));
    const O colb = O(gcol) * O(sizeof(T));
    const O zo = O(threadIdx.x & (kWave - 1)) * O(sizeof(T));   // this lane's word of the zero line
    const auto at_aph = [&](O x) { return (have >> NL_IN_APH & 1u) ? x : zo; };
    const auto slot = [&](int w, int d) -> T& { return s_carry[(w * ndir + d) * kColBlock]; };

    const T trpaus = trpaus_prescan<T, false, O>(F.in(NL_IN_T), F.in(NL_IN_TND_CML_T), lsb, colb, dt, s_eta, klo, khi);
    const CrhCol<T> crh = crh_setup<T>(trpaus);

    // :124-135, :757-765
    TLCarry<T> c = tl_carry_top<T, EVAP, O>(F.in(NL_IN_APH), colb, O(nz) * lsb + colb);
    tl_zero_top_flux<T>(F, want & kTLWantNL, colb);
    for (int d = 0; d < ndir; ++d) {
        const T* aph_i = F.in_i(NL_IN_APH) + ((have >> NL_IN_APH & 1u) ? d * in_ds : int64_t(0));
        slot(0, d) = T(0.0);
        slot(1, d) = T(0.0);
        slot(2, d) = T(0.0);
        slot(3, d) = ldg(aph_i, at_aph(colb));
        slot(4, d) = EVAP ? ldg(aph_i, at_aph(O(nz) * lsb + colb)) : T(0.0);
        tl_zero_top_flux<T>(TLDirFields<T>{F, d * out_ds}, want & ~kTLWantNL, colb);
    }

    // perturbation words of direction d at byte offset o
    const auto load_dir = [&](int d, O o) {
        const int64_t ib = d * in_ds;
        const auto ptr = [&](int f) { return F.in_i(f) + ((have >> f & 1u) ? ib : int64_t(0)); };
        return load_level_masked<T, STEP>(ptr, have, lsb, o, zo);
    };
    O o = colb;
    LevelIn<T> xa = load_level<T, O>(F_in, lsb, o, STEP), ya = load_dir(0, o);
    for (int k = 0; k < nz; ++k) {
        const bool more = k + 1 < nz;
        LevelIn<T> xn = xa;
        if (more) xn = load_level<T, O>(F_in, lsb, o + lsb, STEP);
        T g_t = T(0.0), g_ap = T(0.0);
        if constexpr (STEP) {
            const SatD<T> s = saturation_point_d<T, 0>(e, xk, xa.t, xa.ap);
            xa.qsat = s.qsat;
            g_t = s.g_t;
            g_ap = s.g_ap;
        }
        const T rfl0 = c.rfl, sfl0 = c.sfl, covptot0 = c.covptot, aph_k0 = c.aph_k;
        for (int d = 0; d < ndir; ++d) {
            F.fresh();
            const bool last = d + 1 == ndir;
            const LevelIn<T> yn = load_dir(last ? 0 : d + 1, last && more ? o + lsb : o);
            if constexpr (STEP) ya.qsat = g_t * ya.t + g_ap * ya.ap;
            c.rfl = rfl0; c.sfl = sfl0; c.covptot = covptot0; c.aph_k = aph_k0;
            c.rfl_i = slot(0, d); c.sfl_i = slot(1, d); c.covptot_i = slot(2, d); c.aph_k_i = slot(3, d); c.aph_s_i = slot(4, d);
            const TLOut<T> r = tl_level<T, REG, EVAP>(e, kc, xk, xa, ya, k, s_eta[k], s_scalm[k], crh, dt, c);
            slot(0, d) = c.rfl_i; slot(1, d) = c.sfl_i; slot(2, d) = c.covptot_i; slot(3, d) = c.aph_k_i;
            const TLDirFields<T> Fd{F, d * out_ds};
            tl_store_masked<T>(Fd, d == 0 ? want : want & ~kTLWantNL, e, lsb, o, r);
            drain_vmem();   // see drain_vmem
            ya = yn;
        }
        xa = xn;
        o += lsb;
    }
}

template <typename T, bool REG, bool EVAP>
__global__ void __launch_bounds__(kColBlock)
tl_dirs_kernel(const TLDirsArgs<T> A) {
    tl_dirs_sweep<T, REG, EVAP, false>(A);
}

template <typename T, bool REG, bool EVAP>
__global__ void __launch_bounds__(kColBlock)
tl_dirs_step_kernel(const TLDirsArgs<T> A) {
    tl_dirs_sweep<T, REG, EVAP, true>(A);
}

// launch_tl_masked for `ndir` directions (1 <= ndir <= kTLMaxDirs, checked by the caller): in_i[f] / out_i[f] point at
// direction 0; the strides are in elements
template <typename T>
int launch_tl_dirs(const TLCall<T>& c) {
    if (!fits_u32_offsets<T>(c.nz, c.ls)) return -2;
    const bool step = c.is(kStep);
    TLDirsArgs<T> args;
    args.m = fill_tl_masked_args<T>(c);
    args.in_ds = c.dirs.in_ds; args.out_ds = c.dirs.out_ds; args.ndir = c.dirs.ndir;
    const dim3 grid((c.nx + kColBlock - 1) / kColBlock);
    const size_t smem = tl_dirs_lds_bytes<T>(c.nz, c.dirs.ndir);
    // device_always: the device is looked up whatever the LDS demand (an ordinal beyond kMaxDevices is refused, -2)
    return with_flags(
        [&](auto REG, auto EVAP, auto STEP) {
            constexpr auto kern = STEP ? tl_dirs_step_kernel<T, REG, EVAP> : tl_dirs_kernel<T, REG, EVAP>;
            return launch_tail<kern>({grid, smem, c.stream, step ? "cs2::tl_dirs_step_kernel" : "cs2::tl_dirs_kernel", true}, args);
        },
        c.p->LREGCL != 0, evap_on(*c.p), step);
}

template int launch_tl_dirs<double>(const TLCall<double>&);
template int launch_tl_dirs<float>(const TLCall<float>&);

}  // namespace cs2
