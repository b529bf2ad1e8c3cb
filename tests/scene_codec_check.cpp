// The scene codec (csrc/sb_scene_codec.h) on its own.  Reads a scene dumped by tests/test_hostcheck_cpu.py in the reference's buffer
// layouts and, beside it, what numpy (softbody-webgpu_amd/layout.py) reads from the same buffers per beam slot: endpoints and the nine
// floats, 11 words a slot.  Checks that (1) the codec decodes every record to exactly those words, alone and through the validation
// walk, and that encode followed by decode returns the record; (2) each defect of a scene -- particle index out of range / mapped
// twice, beam index out of range / mapped twice, endpoint not mapped -- planted once in an early and once in a late range of slots
// is reported with the right kind, slot and indices, by the library's own parallel walk and by 1 and 8 threads over explicit ranges;
// (3) of two defects in different ranges the one at the lower slot is reported.  Built with AddressSanitizer + UBSan and with
// ThreadSanitizer by `make hostcheck`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "sb_scene_codec.h"

#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            fprintf(stderr, "scene_codec_check: %s failed (line %d) %s\n", #c, __LINE__, g_what); \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)
static const char *g_what = "";

struct Bufs {
    uint32_t layout = 0, maxP = 0, maxB = 0;
    std::vector<uint8_t> md, mp, pd, bd;
    sbc::Scene scene() const
    {
        const sbc::Header h(md.data());
        return sbc::Scene{layout, maxP, maxB, h.P, h.B, mp.data(), bd.data()};
    }
    uint32_t bmap(uint32_t s) const { return sbc::map_get(layout, mp.data(), (size_t)maxP + s); }
    void set_bmap(uint32_t s, uint32_t v) { sbc::map_set(layout, mp.data(), (size_t)maxP + s, v); }
};

static bool same(const sbc::SceneError &x, const sbc::SceneError &y)
{
    return x.kind == y.kind && x.slot == y.slot && x.idx == y.idx && x.a == y.a && x.b == y.b;
}

// the beam slots in `threads` explicit ranges side by side, reduced as the library does
static sbc::SceneError walk(const Bufs &u, const std::vector<uint32_t> &slot_of_data, unsigned threads)
{
    const sbc::Scene sc = u.scene();
    std::vector<uint32_t> claimed(sc.maxB, sbc::NONE);
    std::vector<sbc::SceneError> per_range(threads);
    std::vector<std::thread> th;
    for (unsigned w = 0; w < threads; w++)
        th.emplace_back([&, w] {
            per_range[w] = sbc::check_beam_range(sc, slot_of_data.data(), claimed.data(), (size_t)sc.B * w / threads, (size_t)sc.B * (w + 1) / threads,
                                                 [](const sbc::BeamSlot &) {});
        });
    for (auto &t : th) t.join();
    sbc::SceneError first;
    for (const sbc::SceneError &e : per_range)
        if (sbc::before(e, first)) first = e;
    return first;
}

// a spoiled scene must be refused with exactly `want`, however it is walked
static int expect(const Bufs &u, const sbc::SceneError &want, const char *what)
{
    g_what = what;
    std::vector<uint32_t> data_of_slot, slot_of_data;
    const sbc::SceneError got = sbc::validate_scene(u.scene(), data_of_slot, slot_of_data, [](const sbc::BeamSlot &) {});
    if (!same(got, want))
        fprintf(stderr, "%s: got kind %u slot %u idx %u a %u b %u, want kind %u slot %u idx %u a %u b %u\n", what, got.kind, got.slot, got.idx, got.a, got.b,
                want.kind, want.slot, want.idx, want.a, want.b);
    CHECK(same(got, want));
    if (want.kind == sbc::PARTICLE_RANGE || want.kind == sbc::PARTICLE_TWICE) return 0; // (the beams are not looked at then)
    for (unsigned threads : {1u, 8u}) CHECK(same(walk(u, slot_of_data, threads), want));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    Bufs u;
    {
        FILE *f = fopen(argv[1], "rb");
        CHECK(f);
        uint32_t head[4]; // layout, max_particles, max_beams, reserved
        CHECK(fread(head, 4, 4, f) == 4);
        u.layout = head[0], u.maxP = head[1], u.maxB = head[2];
        u.md.resize(SB_METADATA_BYTES);
        u.mp.resize(sbc::mapping_bytes(u.layout, u.maxP, u.maxB));
        u.pd.resize((size_t)u.maxP * SB_PARTICLE_STRIDE);
        u.bd.resize((size_t)u.maxB * sbc::beam_stride(u.layout));
        CHECK(fread(u.md.data(), 1, u.md.size(), f) == u.md.size());
        CHECK(fread(u.mp.data(), 1, u.mp.size(), f) == u.mp.size());
        CHECK(fread(u.pd.data(), 1, u.pd.size(), f) == u.pd.size());
        CHECK(fread(u.bd.data(), 1, u.bd.size(), f) == u.bd.size());
        fclose(f);
    }
    const sbc::Header hd(u.md.data());
    const uint32_t P = hd.P, B = hd.B, layout = u.layout, maxP = u.maxP, maxB = u.maxB, stride = sbc::beam_stride(layout);
    CHECK(P >= 64 && B >= 64 && maxP > P && maxB > B); // (the plantings below need room)
    CHECK(hd.capacity_is(maxP, maxB) && hd.counts_fit(maxP, maxB) && !hd.capacity_is(maxP + 1, maxB) && !hd.counts_fit(P, B - 1) && !hd.counts_fit(P - 1, B));
    std::vector<uint32_t> want((size_t)B * 11);
    {
        FILE *f = fopen(argv[2], "rb");
        CHECK(f);
        CHECK(fread(want.data(), 4, want.size(), f) == want.size());
        fclose(f);
    }

    // ---- sizes: every buffer exact, each one a byte short, optional buffers absent
    {
        const size_t n[4] = {u.md.size(), u.mp.size(), u.pd.size(), u.bd.size()};
        CHECK(sbc::check_sizes(layout, maxP, maxB, true, u.md.data(), n[0], u.mp.data(), n[1], u.pd.data(), n[2], u.bd.data(), n[3]).buffer == sbc::BUF_OK);
        for (int k = 0; k < 4; k++) {
            size_t m[4] = {n[0], n[1], n[2], n[3]};
            m[k]--;
            const sbc::SizeError e = sbc::check_sizes(layout, maxP, maxB, true, u.md.data(), m[0], u.mp.data(), m[1], u.pd.data(), m[2], u.bd.data(), m[3]);
            CHECK(e.buffer == sbc::BUF_METADATA + (uint32_t)k && e.have == m[k] && e.need == n[k]);
        }
        CHECK(sbc::check_sizes(layout, maxP, maxB, true, u.md.data(), n[0], nullptr, n[1], u.pd.data(), n[2], u.bd.data(), n[3]).buffer == sbc::BUF_NULL);
        CHECK(sbc::check_sizes(layout, maxP, maxB, false, nullptr, 0, nullptr, 0, u.pd.data(), n[2], nullptr, 0).buffer == sbc::BUF_OK);
        CHECK(sbc::check_sizes(layout, maxP, maxB, false, nullptr, 0, nullptr, 0, nullptr, 0, u.bd.data(), n[3] - 1).buffer == sbc::BUF_BEAMS);
    }

    // ---- (1) decode == numpy's decode; encode . decode == identity; the validation walk hands out the same
    std::vector<uint32_t> data_of_slot, slot_of_data;
    for (uint32_t s = 0; s < B; s++) {
        const uint8_t *rec = u.bd.data() + (size_t)u.bmap(s) * stride, *f9;
        uint32_t a, b;
        sbc::decode_beam(layout, rec, a, b, f9);
        const uint32_t *w = &want[(size_t)s * 11];
        CHECK(a == w[0] && b == w[1] && memcmp(f9, w + 2, 36) == 0);
        uint8_t again[SB_BEAM_STRIDE_V2];
        memset(again, 0xA5, sizeof again);
        sbc::encode_beam(layout, again, a, b, f9);
        CHECK(memcmp(again, rec, stride) == 0);
    }
    {
        std::vector<uint32_t> seen((size_t)B * 13, 0u);
        const sbc::SceneError ok = sbc::validate_scene(u.scene(), data_of_slot, slot_of_data, [&](const sbc::BeamSlot &r) {
            uint32_t *o = &seen[(size_t)r.slot * 13];
            o[0] = r.da, o[1] = r.db, o[11] = r.a, o[12] = r.b;
            memcpy(o + 2, r.f9, 36);
            if (r.idx != u.bmap(r.slot)) o[0] = ~r.da;
        });
        CHECK(ok.kind == sbc::SCENE_OK && data_of_slot.size() == P && slot_of_data.size() == maxP);
        for (uint32_t s = 0; s < P; s++) CHECK(data_of_slot[s] == sbc::map_get(layout, u.mp.data(), s) && slot_of_data[data_of_slot[s]] == s);
        for (uint32_t s = 0; s < B; s++) {
            const uint32_t *o = &seen[(size_t)s * 13], *w = &want[(size_t)s * 11];
            CHECK(memcmp(o, w, 44) == 0 && o[11] == slot_of_data[w[0]] && o[12] == slot_of_data[w[1]]);
        }
        for (unsigned threads : {1u, 8u}) CHECK(walk(u, slot_of_data, threads).kind == sbc::SCENE_OK);
    }
    uint32_t free_p = sbc::NONE, free_b = sbc::NONE; // data indices no slot maps to
    for (uint32_t i = 0; i < maxP && free_p == sbc::NONE; i++)
        if (slot_of_data[i] == sbc::NONE) free_p = i;
    {
        std::vector<uint8_t> used(maxB, 0);
        for (uint32_t s = 0; s < B; s++) used[u.bmap(s)] = 1;
        for (uint32_t i = 0; i < maxB && free_b == sbc::NONE; i++)
            if (!used[i]) free_b = i;
    }
    CHECK(free_p != sbc::NONE && free_b != sbc::NONE);

    // ---- (2) each defect once, in the first and in a late range of slots (with 8 ranges: the first and the seventh)
    auto spoil_endpoint = [&](Bufs &v, uint32_t s, bool second) { // -> the record's endpoints afterwards
        uint8_t *rec = v.bd.data() + (size_t)v.bmap(s) * stride;
        const uint8_t *f9;
        uint32_t a, b;
        sbc::decode_beam(layout, rec, a, b, f9);
        (second ? b : a) = free_p;
        float f[9];
        memcpy(f, f9, sizeof f);
        sbc::encode_beam(layout, rec, a, b, f);
        return std::make_pair(a, b);
    };
    int defects = 0;
    for (int late = 0; late < 2; late++) {
        const uint32_t ps = late ? P / 16 * 13 + 3 : P / 16 + 1, bs = late ? B / 16 * 13 + 3 : B / 16 + 1;
        {
            Bufs v = u;
            sbc::map_set(layout, v.mp.data(), ps, maxP);
            if (layout == SB_LAYOUT_V2 || maxP < 65536u) {
                if (expect(v, {sbc::PARTICLE_RANGE, ps, maxP, 0, 0}, "particle index out of range")) return 1;
                defects++;
            }
        }
        {
            Bufs v = u;
            sbc::map_set(layout, v.mp.data(), ps, data_of_slot[ps - 1]);
            if (expect(v, {sbc::PARTICLE_TWICE, ps, data_of_slot[ps - 1], ps - 1, 0}, "particle index mapped twice")) return 1;
            defects++;
        }
        {
            Bufs v = u;
            v.set_bmap(bs, maxB);
            if (layout == SB_LAYOUT_V2 || maxB < 65536u) {
                if (expect(v, {sbc::BEAM_RANGE, bs, maxB, 0, 0}, "beam index out of range")) return 1;
                defects++;
            }
        }
        {
            Bufs v = u; // the slot takes the index of one far behind it: the LATER of the two is the offender
            const uint32_t other = bs + B / 8;
            v.set_bmap(bs, u.bmap(other));
            if (expect(v, {sbc::BEAM_TWICE, other, u.bmap(other), 0, 0}, "beam index mapped twice (by an earlier slot)")) return 1;
            defects++;
            v = u; // ... and the index of one before it: the slot itself is
            v.set_bmap(bs, u.bmap(bs - 1));
            if (expect(v, {sbc::BEAM_TWICE, bs, u.bmap(bs - 1), 0, 0}, "beam index mapped twice")) return 1;
            defects++;
        }
        for (int second = 0; second < 2; second++) {
            Bufs v = u;
            const auto ab = spoil_endpoint(v, bs, second != 0);
            if (expect(v, {sbc::ENDPOINT, bs, u.bmap(bs), ab.first, ab.second}, "endpoint not mapped")) return 1;
            defects++;
        }
    }

    // ---- (3) two defects in different ranges: the lower slot is reported, whatever its kind
    {
        const uint32_t lo = B / 16 + 1, hi = B / 16 * 13 + 3;
        Bufs v = u;
        const auto ab = spoil_endpoint(v, lo, false);
        v.set_bmap(hi, maxB < 65536u || layout == SB_LAYOUT_V2 ? maxB : u.bmap(hi - 1));
        if (expect(v, {sbc::ENDPOINT, lo, u.bmap(lo), ab.first, ab.second}, "endpoint low, beam index high")) return 1;
        v = u;
        v.set_bmap(lo, u.bmap(lo - 1));
        spoil_endpoint(v, hi, true);
        if (expect(v, {sbc::BEAM_TWICE, lo, u.bmap(lo - 1), 0, 0}, "beam index twice low, endpoint high")) return 1;
        v = u; // two slots share an index whose record has a bad endpoint: the lower slot's endpoint is what a walk in slot order meets first
        v.set_bmap(hi, free_b);
        v.set_bmap(lo, free_b);
        memcpy(v.bd.data() + (size_t)free_b * stride, u.bd.data() + (size_t)u.bmap(lo) * stride, stride);
        {
            uint8_t *rec = v.bd.data() + (size_t)free_b * stride;
            const uint8_t *f9;
            uint32_t a, b;
            sbc::decode_beam(layout, rec, a, b, f9);
            float f[9];
            memcpy(f, f9, sizeof f);
            sbc::encode_beam(layout, rec, free_p, b, f);
        }
        if (expect(v, {sbc::ENDPOINT, lo, free_b, free_p, want[(size_t)lo * 11 + 1]}, "shared index with a bad endpoint")) return 1;
        defects += 3;
    }
    printf("SCENE_CODEC_OK %u particles %u beams %d defects\n", P, B, defects);
    return 0;
}
