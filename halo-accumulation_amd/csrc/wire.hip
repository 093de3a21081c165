// Wire format of EvalProof / Instance / Accumulator: what `#[derive(CanonicalSerialize)]` with
// compressed points would write for the reference's structs (pcdl.rs:22-30, acc.rs:21-28,43-59), field by field in
// declaration order, so that proofs can leave the process in arkworks' own encoding:
//   Fr                 32 bytes, little endian, canonical (not Montgomery)
//   Projective point   33 bytes: x little endian, flags in the top bits of byte 32 (255 + 2 flag bits > 256):
//                      bit 7 = y is the larger of {y, -y}, bit 6 = point at infinity (x = 0)     [group.rs:45-60 hashes the same bytes]
//   usize              u64 little endian
//   Vec<T>             u64 little-endian length, then the elements
//   Option<T>          one byte 0 / 1, then T
//   DensePolynomial    its coefficient Vec (ark-poly strips trailing zero coefficients)
// The reference derives no (de)serialisation for these three structs and no Rust toolchain exists here, so the layout is
// "best known", exactly like the transcript encoding of host_math.hpp (parity unpinned).  Decoding validates
// everything a checked arkworks deserialisation would: canonical field elements, flag bits, points on the curve.
// The single-blob entry points are host-only code: no device is needed or touched.  The batched decoders (halo_*_decode_batch,
// at the end) read every member's structure on the host and decompress the points of the whole batch at once -- on the device
// (decompress.hip) when a context is given and the batch is large enough, else on the host pool.
#include <algorithm>
#include <cstring>

#include "pcdl_internal.hpp"  // (the blob layout: proof_words, instance_words)

namespace halo {
namespace {

using host::Fq;
using host::Fr;
using host::Point;

struct Writer {
    uint8_t *out;
    size_t cap, pos = 0;
    bool ok = true;
    void put(const void *p, size_t n) {
        if (pos + n > cap) { ok = false; return; }
        std::memcpy(out + pos, p, n);
        pos += n;
    }
    void u64le(uint64_t v) { put(&v, 8); }
    void byte(uint8_t v) { put(&v, 1); }
    void scalar(const uint64_t *mont) {
        Fr c = Fr::load(mont).from_mont();
        put(c.l, 32);
    }
    void point(const uint64_t *jac) {
        uint8_t b[33] = {0};
        Point p = Point::load(jac);
        if (p.is_inf()) {
            b[32] = 0x40;
        } else {
            host::Affine a = p.to_affine();
            Fq x = a.x.from_mont(), y = a.y.from_mont(), ny = (-a.y).from_mont();
            std::memcpy(b, x.l, 32);
            if (!Fq::geq(ny.l, y.l)) b[32] |= 0x80;  // y > -y
        }
        put(b, 33);
    }
};

// sqrt in Fq (p = 1 mod 2^32): Tonelli-Shanks with the generator 5 of ark-pallas' FqConfig
bool fq_sqrt(const Fq &a, Fq *root) {
    if (a.is_zero()) { *root = a; return true; }
    // p - 1 = 2^32 * t
    static const uint64_t T[4] = {0x094cf91b992d30edULL, 0x00000000224698fcULL, 0x0ULL, 0x40000000ULL};
    static const Fq Z = Fq::from_u64(5).pow(T);  // generator of the 2^32-torsion
    uint64_t tm1h[4];                            // (t - 1) / 2
    { uint64_t one[4] = {1, 0, 0, 0}, t1[4]; Fq::sub_limbs(t1, T, one); for (int i = 0; i < 4; ++i) tm1h[i] = (t1[i] >> 1) | (i < 3 ? t1[i + 1] << 63 : 0); }
    Fq w = a.pow(tm1h);
    Fq x = a * w, b = x * w, z = Z;  // x = a^((t+1)/2), b = a^t
    int v = 32;
    while (b != Fq::one()) {
        int k = 0;
        Fq b2k = b;
        while (b2k != Fq::one()) { b2k = b2k.sqr(); if (++k == v) return false; }  // not a square
        Fq wz = z;
        for (int j = 0; j < v - k - 1; ++j) wz = wz.sqr();
        z = wz.sqr();
        b = b * z;
        x = x * wz;
        v = k;
    }
    *root = x;
    return true;
}

// a point whose decompression a batched decode has put off: its 33 bytes and where its 12 words go
struct PendingPoint {
    const uint8_t *src;
    uint64_t *dst;
};
// the point of Reader::point on its own: false = rejected
bool decompress_point(const uint8_t *src, uint64_t *jac_out);

struct Reader {
    const uint8_t *in;
    size_t len, pos = 0;
    bool ok = true;
    std::vector<PendingPoint> *defer = nullptr;  // batched decode: points are queued here, unexamined, and count as good
    bool take(void *p, size_t n) {
        if (!ok || pos + n > len) { ok = false; return false; }
        std::memcpy(p, in + pos, n);
        pos += n;
        return true;
    }
    uint64_t u64le() { uint64_t v = 0; take(&v, 8); return v; }
    int byte() { uint8_t v = 0; take(&v, 1); return v; }
    void scalar(uint64_t *mont_out) {
        Fr c;
        if (!take(c.l, 32)) return;
        if (Fr::geq(c.l, host::FrP::M)) { ok = false; return; }  // not canonical
        c.to_mont().store(mont_out);
    }
    void point(uint64_t *jac_out) {
        if (defer) {
            if (ok && pos + 33 <= len) { defer->push_back({in + pos, jac_out}); pos += 33; }
            else ok = false;
            return;
        }
        uint8_t b[33];
        if (!take(b, 33)) return;
        if (!decompress_point(b, jac_out)) ok = false;
    }
};
bool decompress_point(const uint8_t *src, uint64_t *jac_out) {
    uint8_t b[33];
    std::memcpy(b, src, 33);
    uint8_t flags = b[32] & 0xC0;
    b[32] &= 0x3F;
    if (flags == 0xC0) return false;
    if (flags == 0x40) {
        for (int i = 0; i < 33; ++i) if (b[i]) return false;
        Point::infinity().store(jac_out);
        return true;
    }
    if (b[32]) return false;  // x >= 2^256
    Fq xc;
    std::memcpy(xc.l, b, 32);
    if (Fq::geq(xc.l, host::FqP::M)) return false;
    Fq x = xc.to_mont(), y;
    if (!fq_sqrt(x.sqr() * x + Fq::from_u64(5), &y)) return false;  // not on the curve
    Fq yc = y.from_mont(), nyc = (-y).from_mont();
    bool y_larger = !Fq::geq(nyc.l, yc.l);
    if (y_larger != (flags == 0x80)) y = -y;
    if (y.is_zero() && flags == 0x80) return false;
    Point::from_affine(x, y).store(jac_out);
    return true;
}

void write_proof(Writer &w, const uint64_t *pf) {
    size_t lg = (size_t)pf[1];
    w.u64le(lg);
    for (size_t i = 0; i < lg; ++i) w.point(pf + 2 + 12 * i);
    w.u64le(lg);
    for (size_t i = 0; i < lg; ++i) w.point(pf + 2 + 12 * lg + 12 * i);
    const uint64_t *tail = pf + 2 + 24 * lg;
    w.point(tail);        // U
    w.scalar(tail + 12);  // c
    w.byte(pf[0] ? 1 : 0);
    if (pf[0]) w.point(tail + 16);  // C_bar
    w.byte(pf[0] ? 1 : 0);
    if (pf[0]) w.scalar(tail + 28);  // w'
}
// returns lg, or (size_t)-1
size_t read_proof(Reader &r, uint64_t *pf, size_t cap_words) {
    uint64_t lg = r.u64le();
    if (!r.ok || lg > 40 || proof_words(lg) > cap_words) { r.ok = false; return (size_t)-1; }
    std::memset(pf, 0, 8 * proof_words(lg));
    pf[1] = lg;
    for (size_t i = 0; i < lg; ++i) r.point(pf + 2 + 12 * i);
    if (r.u64le() != lg) { r.ok = false; return (size_t)-1; }  // Ls and Rs have one entry per round
    for (size_t i = 0; i < lg; ++i) r.point(pf + 2 + 12 * lg + 12 * i);
    uint64_t *tail = pf + 2 + 24 * lg;
    r.point(tail);
    r.scalar(tail + 12);
    int has_cbar = r.byte();
    if (has_cbar > 1) { r.ok = false; return (size_t)-1; }
    if (has_cbar) r.point(tail + 16); else Point::infinity().store(tail + 16);
    int has_w = r.byte();
    if (has_w > 1 || has_w != has_cbar) { r.ok = false; return (size_t)-1; }  // open() sets both or neither (pcdl.rs:137-173)
    if (has_w) r.scalar(tail + 28);
    pf[0] = (uint64_t)has_cbar;
    return r.ok ? (size_t)lg : (size_t)-1;
}
void write_instance(Writer &w, const uint64_t *q) {
    w.point(q);
    w.u64le(q[12]);
    w.scalar(q + 13);
    w.scalar(q + 17);
    write_proof(w, q + 21);
}
size_t read_instance(Reader &r, uint64_t *q, size_t cap_words) {
    if (cap_words < 21) { r.ok = false; return (size_t)-1; }
    r.point(q);
    q[12] = r.u64le();
    r.scalar(q + 13);
    r.scalar(q + 17);
    if (!r.ok) return (size_t)-1;
    size_t lg = read_proof(r, q + 21, cap_words - 21);
    if (lg == (size_t)-1) return lg;
    if (q[12] + 1 != ((uint64_t)1 << lg)) { r.ok = false; return (size_t)-1; }  // d + 1 = 2^lg: the proof has lg rounds
    return lg;
}

// a blob's own words say how long it is: a corrupted or foreign blob must not send the encoder out of bounds
// (the decoders cap lg at 40 as well)
bool blob_header_ok(const uint64_t *pf) { return pf[0] <= 1 && pf[1] <= 40; }
int bad_blob() { set_error("encode: not an EvalProof blob (hiding flag > 1 or lg > 40)"); return HALO_E_ARG; }

int finish_write(const Writer &w, size_t *len) {
    if (!w.ok) { set_error("encode: output buffer too small"); return HALO_E_ARG; }
    *len = w.pos;
    return HALO_OK;
}
int reject(const char *what) { set_error(std::string("decode: malformed ") + what); return HALO_E_REJECT; }

// The three decoders after their null checks: status and message (set_error) of halo_*_decode; *lg_n on success.  With
// r.defer set the points count as good and the caller judges them afterwards (decode_batch).
enum WireKind { WIRE_PROOF, WIRE_INSTANCE, WIRE_ACCUMULATOR };
const char *const kWireName[3] = {"EvalProof", "Instance", "Accumulator"};
int decode_proof(Reader &r, uint64_t *proof_out, size_t cap_words, size_t *lg_n) {
    size_t lg = read_proof(r, proof_out, cap_words);
    if (lg == (size_t)-1 || !r.ok || r.pos != r.len) return reject("EvalProof");
    *lg_n = lg;
    return HALO_OK;
}
int decode_instance(Reader &r, uint64_t *inst_out, size_t cap_words, size_t *lg_n) {
    size_t lg = read_instance(r, inst_out, cap_words);
    if (lg == (size_t)-1 || !r.ok || r.pos != r.len) return reject("Instance");
    *lg_n = lg;
    return HALO_OK;
}
// Accumulator = Instance fields | pi_V { h: DensePolynomial (<= 2 coefficients, trailing zeros stripped), U, w }
int decode_accumulator(Reader &r, uint64_t *acc_out, size_t cap_words, size_t *lg_n) {
    size_t lg = read_instance(r, acc_out, cap_words);
    if (lg == (size_t)-1 || !r.ok) return reject("Accumulator");
    if (cap_words < instance_words(lg) + 24) { set_error("decode: output buffer too small"); return HALO_E_ARG; }
    uint64_t *piV = acc_out + instance_words(lg);
    std::memset(piV, 0, 24 * 8);
    uint64_t hlen = r.u64le();
    if (!r.ok || hlen > 2) return reject("Accumulator (h has at most two coefficients, acc.rs:192)");
    for (uint64_t k = 0; k < hlen; ++k) r.scalar(piV + 4 * k);
    if (r.ok && hlen && !(piV[4 * (hlen - 1)] | piV[4 * (hlen - 1) + 1] | piV[4 * (hlen - 1) + 2] | piV[4 * (hlen - 1) + 3]))
        return reject("Accumulator (leading coefficient of h is zero)");
    r.point(piV + 8);
    r.scalar(piV + 20);
    if (!r.ok || r.pos != r.len) return reject("Accumulator");
    *lg_n = lg;
    return HALO_OK;
}

// ---- halo_*_decode_batch
// Member i = in[offs[i], offs[i + 1]) -> out + i * stride, every member's outcome the single call's with cap_words = stride:
//  1. one pool pass over the members reads each one's structure (lengths, option tags, the lg cap, canonical scalars, the
//     accumulator's h) with its points queued, not examined (Reader::defer);
//  2. the queued points of the whole batch are decompressed: by k_point_decompress (decompress.hip) on a slot idle at entry,
//     in chunks of what the context's staging holds, from kDecodeBatchMin finite points on; with no context, no idle slot,
//     no staging or fewer points, by the host pool, point by point;
//  3. a member one of whose queued points was rejected is "malformed <kind>" -- the single call reads in byte order and
//     stops at the first failure, a member's points are queued only up to its first structural failure, and every failure
//     a bad point can precede is reported in those words or after it (the accumulator's "output buffer too small" and its
//     messages about h come after the Instance part; after U only the generic message is left).
constexpr size_t kDecodeBatchMin = 512;          // finite points; measured: tools/time_decode_batch.py
constexpr size_t kDecodeChunk = (size_t)1 << 16;  // points per launch the staging is asked for
constexpr size_t kDecompBytes = (DECOMP_IN_WORDS + DECOMP_OUT_WORDS) * 8;

struct DecodeMember {
    int rc = HALO_OK;
    std::string err;
    size_t lg = 0, first = 0;
    std::vector<PendingPoint> pts;
};

// ok[j] = point j accepted (its words written); returns non-zero only for a failing HIP call
int decompress_on_device(halo_ctx *ctx, int slot, size_t chunk, const std::vector<PendingPoint> &pts, std::vector<uint8_t> &ok) {
    const uint32_t *tab = sqrt_tables_host();
    uint64_t *d_tab = ctx->d_check_stage, *d_in = d_tab + SQRT_TAB_WORDS / 2, *d_out = d_in + chunk * DECOMP_IN_WORDS;
    int rc;
    {
        StreamGuard on_slot(ctx, ctx->streams[slot]);  // (the launch macro uses ctx->stream: the slot's own)
        std::vector<uint64_t> hin(chunk * DECOMP_IN_WORDS), hout(chunk * DECOMP_OUT_WORDS);
        hipError_t e = hipMemcpyAsync(d_tab, tab, SQRT_TAB_WORDS * 4, hipMemcpyHostToDevice, ctx->stream);
        rc = e == hipSuccess ? HALO_OK : hip_fail(e, "hipMemcpyAsync");
        for (size_t lo = 0; lo < pts.size() && !rc; lo += chunk) {
            const size_t cnt = std::min(chunk, pts.size() - lo);
            std::fill(hin.begin(), hin.begin() + cnt * DECOMP_IN_WORDS, 0);
            for (size_t j = 0; j < cnt; ++j) std::memcpy(&hin[j * DECOMP_IN_WORDS], pts[lo + j].src, 33);
            if ((e = hipMemcpyAsync(d_in, hin.data(), cnt * DECOMP_IN_WORDS * 8, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
            if (!rc) rc = point_decompress_dev(ctx, d_in, cnt, reinterpret_cast<const uint32_t *>(d_tab), d_out);
            if (!rc && (e = hipMemcpyAsync(hout.data(), d_out, cnt * DECOMP_OUT_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
            e = hipStreamSynchronize(ctx->stream);  // (also on failure: the host buffers are reused and go with this call)
            if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
            for (size_t j = 0; j < cnt && !rc; ++j) {
                const uint64_t *o = &hout[j * DECOMP_OUT_WORDS];
                ok[lo + j] = o[12] == 1;
                if (ok[lo + j]) std::memcpy(pts[lo + j].dst, o, 96);
            }
        }
    }
    bool busy = false;
    for (int k = 0; k < HALO_SLOTS; ++k) busy = busy || ctx->wss[k].in_flight;
    if (!rc && ctx->prof.on && !busy) ctx->prof.collect();
    return rc;
}

int decode_batch(halo_ctx *ctx, WireKind kind, const uint8_t *in, const size_t *offs, size_t m, uint64_t *out, size_t stride, size_t *lg_out, int *status) {
    if (m == 0) return HALO_OK;
    if (!in || !offs || !out) { set_error("decode_batch: null pointer"); return HALO_E_ARG; }
    for (size_t i = 0; i < m; ++i)
        if (offs[i + 1] < offs[i]) { set_error("decode_batch: offsets must not decrease"); return HALO_E_ARG; }
    if (ctx) {
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    }
    // 1. the structure of every member
    std::vector<DecodeMember> mem(m);
    pool_run(m, [&](size_t i) {
        DecodeMember &M = mem[i];
        uint64_t *slot = out + i * stride;
        std::memset(slot, 0, stride * 8);
        Reader r{in + offs[i], offs[i + 1] - offs[i]};
        r.defer = &M.pts;
        M.rc = kind == WIRE_PROOF ? decode_proof(r, slot, stride, &M.lg) : kind == WIRE_INSTANCE ? decode_instance(r, slot, stride, &M.lg) : decode_accumulator(r, slot, stride, &M.lg);
        if (M.rc) M.err = halo_last_error();
    });
    std::vector<PendingPoint> pts;
    size_t finite = 0;
    for (size_t i = 0; i < m; ++i) {
        mem[i].first = pts.size();
        for (const PendingPoint &p : mem[i].pts) { pts.push_back(p); finite += !(p.src[32] & 0x40); }
    }
    // 2. every point
    std::vector<uint8_t> ok(pts.size(), 0);
    int slot = -1;
    size_t chunk = 0;
    if (ctx && !pts.empty() && sqrt_tables_host()) {
        int idle[HALO_SLOTS];
        if (idle_slots(ctx, idle)) slot = idle[0];
        const long forced = dev_hooks().decode_min;  // (development library: the threshold sweep of tools/time_decode_batch.py)
        const size_t min_pts = forced >= 1 ? (size_t)forced : kDecodeBatchMin;
        const size_t tab_units = (SQRT_TAB_WORDS * 4 + kDecompBytes - 1) / kDecompBytes;  // the tables in front, in units of a point's staging
        if (slot >= 0 && finite >= min_pts) {
            const size_t have = check_stage(ctx, std::min(pts.size(), kDecodeChunk) + tab_units, kDecompBytes);
            if (have > tab_units) chunk = std::min(have - tab_units, kDecodeChunk);
        }
    }
    if (chunk) {
        int rc = decompress_on_device(ctx, slot, chunk, pts, ok);
        if (rc) return rc;
    } else {
        pool_run(pts.size(), [&](size_t j) { ok[j] = decompress_point(pts[j].src, pts[j].dst); });
    }
    // 3. every member's status
    for (size_t i = 0; i < m; ++i) {
        DecodeMember &M = mem[i];
        for (size_t j = 0; j < M.pts.size(); ++j)
            if (!ok[M.first + j]) { M.rc = HALO_E_REJECT; M.err = std::string("decode: malformed ") + kWireName[kind]; break; }
        if (lg_out) lg_out[i] = M.rc ? 0 : M.lg;
    }
    return report_members("member", m, [&](size_t i) { return mem[i].rc; }, [&](size_t i) { return mem[i].err; }, status,
                          [&](size_t i) { std::memset(out + i * stride, 0, stride * 8); });
}

}  // namespace
}  // namespace halo

using namespace halo;

extern "C" {

size_t halo_proof_encoded_size(size_t lg_n, int hiding) { return 8 + 33 * lg_n + 8 + 33 * lg_n + 33 + 32 + 1 + (hiding ? 33 : 0) + 1 + (hiding ? 32 : 0); }
size_t halo_instance_encoded_size(size_t lg_n, int hiding) { return 33 + 8 + 32 + 32 + halo_proof_encoded_size(lg_n, hiding); }
// largest case: both h coefficients present
size_t halo_accumulator_encoded_size(size_t lg_n) { return halo_instance_encoded_size(lg_n, 1) + 8 + 64 + 33 + 32; }

int halo_proof_encode(const uint64_t *proof, uint8_t *out, size_t cap, size_t *len) {
    if (!proof || !out || !len) { set_error("encode: null pointer"); return HALO_E_ARG; }
    if (!blob_header_ok(proof)) return bad_blob();
    Writer w{out, cap};
    write_proof(w, proof);
    return finish_write(w, len);
}
int halo_proof_decode(const uint8_t *in, size_t len, uint64_t *proof_out, size_t cap_words, size_t *lg_n) {
    if (!in || !proof_out || !lg_n) { set_error("decode: null pointer"); return HALO_E_ARG; }
    Reader r{in, len};
    return decode_proof(r, proof_out, cap_words, lg_n);
}
int halo_instance_encode(const uint64_t *inst, uint8_t *out, size_t cap, size_t *len) {
    if (!inst || !out || !len) { set_error("encode: null pointer"); return HALO_E_ARG; }
    if (!blob_header_ok(inst + 21)) return bad_blob();
    Writer w{out, cap};
    write_instance(w, inst);
    return finish_write(w, len);
}
int halo_instance_decode(const uint8_t *in, size_t len, uint64_t *inst_out, size_t cap_words, size_t *lg_n) {
    if (!in || !inst_out || !lg_n) { set_error("decode: null pointer"); return HALO_E_ARG; }
    Reader r{in, len};
    return decode_instance(r, inst_out, cap_words, lg_n);
}
// Accumulator = Instance fields | pi_V { h: DensePolynomial (<= 2 coefficients, trailing zeros stripped), U, w }
int halo_accumulator_encode(const uint64_t *acc, uint8_t *out, size_t cap, size_t *len) {
    if (!acc || !out || !len) { set_error("encode: null pointer"); return HALO_E_ARG; }
    if (!blob_header_ok(acc + 21)) return bad_blob();
    Writer w{out, cap};
    write_instance(w, acc);
    size_t lg = (size_t)acc[22];
    const uint64_t *piV = acc + instance_words(lg);
    bool z1 = !(piV[4] | piV[5] | piV[6] | piV[7]), z0 = !(piV[0] | piV[1] | piV[2] | piV[3]);
    uint64_t hlen = z1 ? (z0 ? 0 : 1) : 2;
    w.u64le(hlen);
    for (uint64_t k = 0; k < hlen; ++k) w.scalar(piV + 4 * k);
    w.point(piV + 8);
    w.scalar(piV + 20);
    return finish_write(w, len);
}
int halo_accumulator_decode(const uint8_t *in, size_t len, uint64_t *acc_out, size_t cap_words, size_t *lg_n) {
    if (!in || !acc_out || !lg_n) { set_error("decode: null pointer"); return HALO_E_ARG; }
    Reader r{in, len};
    return decode_accumulator(r, acc_out, cap_words, lg_n);
}

int halo_proof_decode_batch(halo_ctx *ctx, const uint8_t *in, const size_t *offs, size_t m, uint64_t *out, size_t stride_words, size_t *lg_out, int *status) {
    return decode_batch(ctx, WIRE_PROOF, in, offs, m, out, stride_words, lg_out, status);
}
int halo_instance_decode_batch(halo_ctx *ctx, const uint8_t *in, const size_t *offs, size_t m, uint64_t *out, size_t stride_words, size_t *lg_out, int *status) {
    return decode_batch(ctx, WIRE_INSTANCE, in, offs, m, out, stride_words, lg_out, status);
}
int halo_accumulator_decode_batch(halo_ctx *ctx, const uint8_t *in, const size_t *offs, size_t m, uint64_t *out, size_t stride_words, size_t *lg_out, int *status) {
    return decode_batch(ctx, WIRE_ACCUMULATOR, in, offs, m, out, stride_words, lg_out, status);
}

}  // extern "C"
