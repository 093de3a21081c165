// The succinct check's Fiat-Shamir transcripts of m Instances on the device (pcdl.rs:272-296: C', xi_0 .. xi_lg), bit for bit what
// succinct_challenges (pcdl_acc.hip) computes on the host pool, in four launches on ctx->stream:
//
//   k_transcript_points   one lane per point of a member (C, L_0 .., R_0 .., U, C_bar): its compressed encoding and the verdict
//                         on-curve / invalid / not normalised (transcript_lane.hpp point_compress_lane)
//   k_transcript_head     one lane per member: the scalars' range checks, the member's status in the host's order (instance
//                         before proof), a = rho_0(C, z, v, C_bar) and the three terms (C, 1), (C_bar, a), (S, r - w') of C'
//   k_batch_small_msm     (small_sums.hip, K = 3) C' in Jacobian form; a non-hiding member has two dead terms
//   k_transcript_chain    one lane per member: C' normalised with the shared-inversion routine of curve.hpp, xi_0 = rho_0(C', z, v),
//                         xi_(i+1) = rho_0(xi_i, L_i, R_i) over the compressed points
//
// The header checks that fix a member's layout (d, proof length, flag word) stay on the host; a member that fails one, and a
// member with a point whose Z is neither 0 nor 1 (foreign input: the library writes normalised points), runs on the host pool as
// before, so every member's code and message are the host's under either route.  Every lane touches its own words only.
#include "curve.hpp"
#include "pcdl_internal.hpp"
#include "transcript_lane.hpp"

namespace halo {

using host::Fr;
using host::Point;

// a member's status word in the staging: what the host wrote (live / not the device's), then what the kernels found
constexpr uint64_t TR_OK = 0, TR_BAD_INSTANCE = 1, TR_BAD_PROOF = 2, TR_ZERO_CHALLENGE = 3, TR_HOST = 5, TR_SKIP = 6;

struct TrPoint { uint64_t w[8]; };  // arkworks affine words of a public point, by value

// slot s of a member's 2 lg + 3 points -> its words in the Instance blob q
HALO_DEV const uint64_t *tr_slot_words(const uint64_t *q, uint32_t s, uint32_t lg) {
    const uint64_t *pf = q + 21;
    if (s == 0) return q;
    if (s <= 2 * lg) return pf + 2 + 12 * (size_t)(s - 1);  // L_0 .. L_(lg-1), R_0 .. R_(lg-1): contiguous in the proof
    return s == 2 * lg + 1 ? pf + 2 + 24 * (size_t)lg : pf + 2 + 24 * (size_t)lg + 16;
}

__global__ __launch_bounds__(256) void k_transcript_points(const uint64_t *__restrict__ blobs, size_t stride, const uint64_t *__restrict__ status,
                                                           uint32_t m, uint32_t lg, uint64_t *__restrict__ comp) {
    const uint32_t S = 2 * lg + 3;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)m * S) return;
    const uint32_t i = (uint32_t)(t / S), s = (uint32_t)(t % S);
    if (status[i] != TR_OK) return;
    uint64_t o[TR_POINT_WORDS];
    point_compress_lane(tr_slot_words(blobs + (size_t)i * stride, s, lg), o);
#pragma unroll
    for (int k = 0; k < 5; k++) comp[TR_POINT_WORDS * t + k] = o[k];
}

__global__ __launch_bounds__(64) void k_transcript_head(const uint64_t *__restrict__ blobs, size_t stride, const uint64_t *__restrict__ comp, uint32_t m,
                                                        uint32_t lg, TrPoint S_pub, uint64_t *__restrict__ status, uint64_t *__restrict__ pts,
                                                        uint64_t *__restrict__ sc) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x, S = 2 * lg + 3;
    if (i >= m) return;
    uint64_t *mp = pts + 24 * (size_t)i, *ms = sc + 12 * (size_t)i;
    for (int k = 0; k < 24; k++) mp[k] = 0;  // (a rejected member, a dead term: infinity times zero)
    for (int k = 0; k < 12; k++) ms[k] = 0;
    if (status[i] != TR_OK) return;
    const uint64_t *q = blobs + (size_t)i * stride, *pf = q + 21, *tail = pf + 2 + 24 * (size_t)lg;  // tail: U | c | C_bar | w'
    const uint64_t *mc = comp + TR_POINT_WORDS * (size_t)i * S;
    const bool hiding = pf[0] == 1;
    const Fe z = fe_load64(q + 13), v = fe_load64(q + 17), wp = fe_load64(tail + 28);
    auto verdict = [&](uint32_t s) { return (uint32_t)(mc[TR_POINT_WORDS * (size_t)s + 4] >> 8); };
    bool foreign = verdict(0) == TR_FOREIGN, bad_proof = false;
    const bool bad_instance = verdict(0) == TR_INVALID || !scalar_ok_lane(z) || !scalar_ok_lane(v);
    const uint32_t live = hiding ? S : S - 1;  // (the C_bar slot is dead for a non-hiding member)
    for (uint32_t s = 1; s < live; s++) {
        const uint32_t vd = verdict(s);
        foreign = foreign || vd == TR_FOREIGN;
        bad_proof = bad_proof || vd == TR_INVALID;
    }
    bad_proof = bad_proof || !scalar_ok_lane(fe_load64(tail + 12)) || (hiding && !scalar_ok_lane(wp));
    const uint64_t st = foreign ? TR_HOST : bad_instance ? TR_BAD_INSTANCE : bad_proof ? TR_BAD_PROOF : TR_OK;
    status[i] = st;
    if (st != TR_OK) return;
    // (C, 1): the blob's own (x, y), or (0, 0) for infinity
    if ((mc[4] & 0xFFu) != 0x40u)
        for (int k = 0; k < 8; k++) mp[k] = q[k];
    ms[0] = 1;
    if (hiding) {
        const uint64_t *cb = mc + TR_POINT_WORDS * (size_t)(S - 1);
        const Fe a = rho0_C_z_v_Cbar(mc, z, v, cb);
        if ((cb[4] & 0xFFu) != 0x40u)
            for (int k = 0; k < 8; k++) mp[8 + k] = tail[16 + k];
        fe_store64(ms + 4, fe_from_mont<FrCfg>(a));
        for (int k = 0; k < 8; k++) mp[16 + k] = S_pub.w[k];
        fe_store64(ms + 8, fe_neg<FrCfg>(fe_from_mont<FrCfg>(wp)));
    }
}

__global__ __launch_bounds__(64) void k_transcript_chain(const uint64_t *__restrict__ blobs, size_t stride, const uint64_t *__restrict__ comp, uint32_t m,
                                                         uint32_t lg, uint64_t *__restrict__ status, uint64_t *__restrict__ cprime,
                                                         uint64_t *__restrict__ xis) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x, S = 2 * lg + 3;
    if (i >= m) return;
    uint64_t *cp = cprime + 12 * (size_t)i, *mx = xis + 4 * (size_t)i * (lg + 1);
    if (status[i] != TR_OK) {
        for (int k = 0; k < 12; k++) cp[k] = 0;
        for (uint32_t k = 0; k < 4 * (lg + 1); k++) mx[k] = 0;
        return;
    }
    const uint64_t *q = blobs + (size_t)i * stride;
    const uint64_t *mc = comp + TR_POINT_WORDS * (size_t)i * S;
    JacN p[1] = {jac_from_words(cp)};
    AffN a[1];
    jac_batch_to_aff(p, a);
    const bool inf = aff_is_inf(a[0]);
    const Fe one = fe_one<FqCfg>();
    const Fe x = inf ? one : fq_to_words(a[0].x), y = inf ? one : fq_to_words(a[0].y);
    fe_store64(cp, x);
    fe_store64(cp + 4, y);
    fe_store64(cp + 8, inf ? fe_zero() : one);
    uint64_t cc[TR_POINT_WORDS];
    point_compress_xy(x, y, inf, cc);
    Fe xi = rho0_C_z_v(cc, fe_load64(q + 13), fe_load64(q + 17));
    fe_store64(mx, xi);
    bool zero = false;  // (host: the check follows each round's challenge, xi_0 is not tested)
#pragma unroll 1
    for (uint32_t j = 0; j < lg; j++) {
        xi = rho0_xi_L_R(xi, mc + TR_POINT_WORDS * (size_t)(1 + j), mc + TR_POINT_WORDS * (size_t)(1 + lg + j));
        zero = zero || fe_is_zero(xi);
        fe_store64(mx + 4 * (size_t)(j + 1), xi);
    }
    if (zero) status[i] = TR_ZERO_CHALLENGE;
}

static void transcript_on_host(halo_ctx *ctx, const uint64_t *q, BatchCheck *r) {
    r->rc = succinct_challenges(ctx, Point::load(q), (size_t)q[12], Fr::load(q + 13), Fr::load(q + 17), q + 21, &r->st, false);
    if (r->rc) r->err = halo_last_error();
}

int transcripts_batch_dev(halo_ctx *ctx, size_t d, const BlobAt &blob_at, size_t m, std::vector<BatchCheck> &res, bool need_relation_inputs) {
    res.assign(m, BatchCheck());
    if (m == 0) return HALO_OK;
    if (m > 0xFFFFFFFFu / 256) { set_error("transcripts_batch: too many members"); return HALO_E_ARG; }
    const bool shape_ok = is_pow2(d + 1) && d + 1 <= ctx->n;
    const size_t lg = shape_ok ? ilog2(d + 1) : 0, S = 2 * lg + 3, iw = instance_words(lg);
    // the checks that fix a member's layout: a member failing one is the host's (its message is the host's, in the host's order)
    std::vector<uint64_t> status(m, TR_SKIP);
    std::vector<size_t> host_members;
    for (size_t i = 0; i < m; ++i) {
        const uint64_t *q = blob_at(i);
        if (shape_ok && q[12] == d && q[22] == lg && q[21] <= 1) status[i] = TR_OK;
        else host_members.push_back(i);
    }
    if (host_members.size() < m) {
        // the blobs as the caller holds them if they lie at one stride, else packed; every region starts at an even word
        size_t stride = m > 1 ? (size_t)(blob_at(1) - blob_at(0)) : iw;
        bool strided = m == 1 || (blob_at(1) > blob_at(0) && stride >= iw);
        for (size_t i = 2; i < m && strided; ++i) strided = blob_at(i) == blob_at(0) + i * stride;
        if (!strided) stride = iw;
        const size_t blob_words = (m - 1) * stride + iw;
        const size_t o_pts = (blob_words + 1) & ~(size_t)1, o_sc = o_pts + m * 24, o_cp = o_sc + m * 12, o_xis = o_cp + m * 12,
                     o_comp = o_xis + m * 4 * (lg + 1), o_st = o_comp + m * S * TR_POINT_WORDS, total = o_st + m;
        if (check_stage(ctx, 1, total * 8) < 1) return kTranscriptNoStage;
        uint64_t *dv = ctx->d_check_stage;
        std::vector<uint64_t> packed;
        const uint64_t *src = blob_at(0);
        if (!strided) {
            packed.resize(blob_words);
            for (size_t i = 0; i < m; ++i)
                if (status[i] == TR_OK) std::memcpy(&packed[i * iw], blob_at(i), iw * 8);
            src = packed.data();
        }
        HALO_HIP(hipMemcpyAsync(dv, src, blob_words * 8, hipMemcpyHostToDevice, ctx->stream));
        HALO_HIP(hipMemcpyAsync(dv + o_st, status.data(), m * 8, hipMemcpyHostToDevice, ctx->stream));
        static const Point kS = public_s_table().mul(Fr::one()).normalized();
        TrPoint s_pub;
        kS.X.store(s_pub.w);
        kS.Y.store(s_pub.w + 4);
        const dim3 per_member((unsigned)((m + 63) / 64)), wave(64);
        HALO_LAUNCH(ctx, "k_transcript_points", k_transcript_points, dim3((unsigned)((m * S + 255) / 256)), dim3(256), 0, dv, stride, dv + o_st, (uint32_t)m,
                    (uint32_t)lg, dv + o_comp);
        HALO_LAUNCH(ctx, "k_transcript_head", k_transcript_head, per_member, wave, 0, dv, stride, dv + o_comp, (uint32_t)m, (uint32_t)lg, s_pub, dv + o_st,
                    dv + o_pts, dv + o_sc);
        HALO_HIP(hipGetLastError());
        int rc = batch_small_msm(ctx, dv + o_pts, dv + o_sc, m, 3, dv + o_cp);
        if (rc) return rc;
        HALO_LAUNCH(ctx, "k_transcript_chain", k_transcript_chain, per_member, wave, 0, dv, stride, dv + o_comp, (uint32_t)m, (uint32_t)lg, dv + o_st, dv + o_cp,
                    dv + o_xis);
        HALO_HIP(hipGetLastError());
        std::vector<uint64_t> back(o_comp - o_cp);  // C' | xis
        HALO_HIP(hipMemcpyAsync(back.data(), dv + o_cp, back.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HALO_HIP(hipMemcpyAsync(status.data(), dv + o_st, m * 8, hipMemcpyDeviceToHost, ctx->stream));
        HALO_HIP(hipStreamSynchronize(ctx->stream));
        int idle[HALO_SLOTS];
        if (ctx->prof.on && idle_slots(ctx, idle) == HALO_SLOTS) ctx->prof.collect();  // (nothing of the caller's in flight to wait for)
        const uint64_t *cps = back.data(), *xs = back.data() + m * 12;
        for (size_t i = 0; i < m; ++i) {
            BatchCheck &r = res[i];
            switch (status[i]) {
                case TR_OK: {
                    r.st.lg_n = lg;
                    r.st.C_prime = Point::load(cps + 12 * i);
                    r.st.xis.resize(lg + 1);
                    for (size_t k = 0; k <= lg; ++k) r.st.xis[k] = Fr::load(xs + (i * (lg + 1) + k) * 4);
                    if (need_relation_inputs) r.st.U = Point::load(pf_U(const_cast<uint64_t *>(blob_at(i)) + 21, lg));
                    break;
                }
                case TR_BAD_INSTANCE: r.rc = HALO_E_REJECT; r.err = "instance holds an invalid point or scalar"; break;
                case TR_BAD_PROOF: r.rc = HALO_E_REJECT; r.err = "proof holds an invalid point or scalar"; break;
                case TR_ZERO_CHALLENGE: r.rc = HALO_E_REJECT; r.err = "challenge is zero"; break;
                case TR_HOST: host_members.push_back(i); break;
                default: break;  // TR_SKIP: in host_members already
            }
        }
    }
    pool_run(host_members.size(), [&](size_t k) { transcript_on_host(ctx, blob_at(host_members[k]), &res[host_members[k]]); });
    return HALO_OK;
}

// The one rule of the batched calls' transcripts: on the device from transcript_min members on (the hook, else the measured
// default) where the context batches its verifier work and the optional staging is to be had, else the host pool.
int transcripts_batch(halo_ctx *ctx, size_t d, const BlobAt &blob_at, size_t m, std::vector<BatchCheck> &res) {
    const long forced = dev_hooks().transcript_min;
    const size_t min = forced >= 1 ? (size_t)forced : kTranscriptMin;
    if (ctx->batch_verify && m >= min) {
        int rc = transcripts_batch_dev(ctx, d, blob_at, m, res, true);
        if (rc != kTranscriptNoStage) return rc;
    }
    res.assign(m, BatchCheck());
    pool_run(m, [&](size_t i) { transcript_on_host(ctx, blob_at(i), &res[i]); });
    return HALO_OK;
}

}  // namespace halo
