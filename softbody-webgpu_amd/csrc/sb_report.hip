// sb_report.hip -- what the engine's state calls and its four whole-scene reports share (sb_report.h; gfx950, wave64).
#include <algorithm>
#include <chrono>

#include "sb_report.h"

// ---------------------------------------------------------------- device buffers

sb_status SbDevBuf::grow(sb_engine *e, size_t bytes)
{
    bytes = std::max<size_t>(bytes, 16);
    if (p && cap >= bytes) return SB_OK;
    if (p) {
        SB_HIP(e, hipStreamSynchronize(e->stream)); // a call in flight may still use it
        SB_HIP(e, hipFree(p));
        p = nullptr;
        cap = 0;
    }
    SB_HIP(e, hipMalloc(&p, bytes));
    cap = bytes;
    return SB_OK;
}

void SbDevBuf::release()
{
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

void sbs_invalidate(sb_engine *e)
{
    if (e && e->sio) e->sio->invalidate();
}

void sbs_release(sb_engine *e)
{
    if (!e || !e->sio) return;
    for (SbDevBuf &b : e->sio->buf) b.release();
    delete e->sio;
    e->sio = nullptr;
}

// ---------------------------------------------------------------- the host mirror

sb_status SbqMirror::stage(SbReportBuf buf, const void *caller, size_t bytes, size_t cap_bytes, bool upload)
{
    SbDevBuf &b = e->sio->buf[buf];
    SB_TRY(b.grow(e, cap_bytes));
    if (upload) SB_HIP(e, hipMemcpyAsync(b.p, caller, bytes, hipMemcpyHostToDevice, e->stream));
    return SB_OK;
}

void *SbqMirror::bind(SbReportBuf buf, void *caller, size_t bytes, size_t cap_bytes, bool upload, bool download)
{
    if (!host || !caller) return caller;
    if (st == SB_OK) st = stage(buf, caller, bytes, cap_bytes, upload);
    if (st != SB_OK) return nullptr;
    void *dev = e->sio->buf[buf].p;
    if (download) back.push_back({caller, dev, bytes});
    return dev;
}

sb_status SbqMirror::finish()
{
    if (!host) return SB_OK;
    for (const Copy &c : back) SB_HIP(e, hipMemcpyAsync(c.caller, c.dev, c.bytes, hipMemcpyDeviceToHost, e->stream));
    SB_HIP(e, hipStreamSynchronize(e->stream));
    return SB_OK;
}

// ---------------------------------------------------------------- preflight, kernel resources

sb_status sbq_ready(sb_engine *e, const char *what, const char *why)
{
    if (!e->loaded) SB_FAIL(e, SB_ERR_STATE, "%s before sb_write_buffers", what);
    if (sb_has_ranks(e)) SB_FAIL(e, SB_ERR_UNSUPPORTED, "%s: the engine has ghost zones or peers configured (%s)", what, why);
    SB_HIP(e, hipSetDevice(e->device));
    if (!e->sio) e->sio = new SbStateIoState();
    return SB_OK;
}

bool sbq_kernel_most(sb_engine *e, const std::vector<const void *> &kernels, bool want_vgprs, uint64_t *value)
{
    uint64_t most = 0;
    for (const void *f : kernels) {
        hipFuncAttributes fa{};
        if (hipSetDevice(e->device) != hipSuccess || hipFuncGetAttributes(&fa, f) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        most = std::max<uint64_t>(most, want_vgprs ? (uint64_t)fa.numRegs : (uint64_t)fa.localSizeBytes);
    }
    *value = most;
    return true;
}

// ---------------------------------------------------------------- the scene tables of the latest upload

static double sbq_ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Every upload path fills h_copy_of_slot for every engine slot (sb_api.hip: layout_blocked, layout_tiled, layout_atomic, and the
// plan-keeping rewrite), so the fourth plane could always be built; it is built when a report asks for it (SBQ_COPIES: body summary
// alone), since sb_bodies would pay a quarter more host work and upload for a plane it never reads.  The block holds all four.
sb_status sbq_need(sb_engine *e, const char *what, uint32_t parts)
{
    SbStateIoState &s = *e->sio;
    if ((parts & SBQ_BEAMS) && !s.beam_valid) parts |= SBQ_PARTICLES; // (the endpoint check reads part 1 on the host)
    if ((parts & SBQ_PARTICLES) && !s.part_valid) {
        const auto t0 = std::chrono::steady_clock::now();
        if (e->h_pidx.size() != e->P) SB_FAIL(e, SB_ERR_STATE, "%s: host shadows of the scene are inconsistent", what);
        const sbq::Defect d = sbq::invert_particles(e->h_pidx.data(), e->P, e->opt.max_particles, s.h_pinv, &s.np);
        if (d != sbq::OK) SB_FAIL(e, SB_ERR_STATE, "%s: %s", what, sbq::defect_text(d));
        SB_TRY(s.buf[SBQ_B_PINV].grow(e, s.h_pinv.size() * sizeof(uint32_t)));
        SB_HIP(e, hipMemcpyAsync(s.buf[SBQ_B_PINV].p, s.h_pinv.data(), s.h_pinv.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        SB_HIP(e, hipStreamSynchronize(e->stream)); // (h_pinv may be rebuilt by the next upload's first call)
        s.P = e->P;
        s.part_valid = true;
        s.beam_valid = s.copy_valid = false;
        s.part_ms = sbq_ms_since(t0);
    }
    const unsigned planes = ((parts & SBQ_BEAMS) && !s.beam_valid ? sbq::ENDS : 0u) | ((parts & SBQ_COPIES) && !s.copy_valid ? sbq::COPY : 0u);
    if (planes) {
        const auto t0 = std::chrono::steady_clock::now();
        if (e->h_beams.size() != e->B || e->h_copy_of_slot.size() < e->B) SB_FAIL(e, SB_ERR_STATE, "%s: host shadows of the scene are inconsistent", what);
        const uint32_t nslots = sb_user_beams(e);
        const size_t n = std::max<uint32_t>(nslots, 1);
        std::vector<uint32_t> tab;
        const sbq::Defect d = sbq::beam_planes(planes, e->h_user_slot.empty() ? nullptr : e->h_user_slot.data(), nslots, e->h_beams.data(),
                                               e->h_copy_of_slot.data(), e->B, e->nbeam, s.h_pinv, s.np, tab);
        if (d != sbq::OK) SB_FAIL(e, SB_ERR_STATE, "%s: %s", what, sbq::defect_text(d));
        SB_TRY(s.buf[SBQ_B_TAB].grow(e, 4 * n * sizeof(uint32_t))); // (the same size for either build of one upload: nothing uploaded is lost)
        uint32_t *to = s.buf[SBQ_B_TAB].as<uint32_t>() + ((planes & sbq::ENDS) ? 0 : 3 * n);
        SB_HIP(e, hipMemcpyAsync(to, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        SB_HIP(e, hipStreamSynchronize(e->stream)); // (the host vector goes out of scope)
        s.nslots = nslots;
        // each plane set's own time; built in one pass, the time is the ends' and the copies cost nothing more
        if (planes & sbq::COPY) s.copy_valid = true, s.copy_ms = (planes & sbq::ENDS) ? 0.0 : sbq_ms_since(t0);
        if (planes & sbq::ENDS) s.beam_valid = true, s.beam_ms = sbq_ms_since(t0);
    }
    if ((parts & SBQ_SLOTS) && !s.islot_valid) { // sb_forces.hip: mapping slot -> internal particle, the sibling of part 1
        const auto t0 = std::chrono::steady_clock::now();
        if (e->h_pslot.size() != e->P) SB_FAIL(e, SB_ERR_STATE, "%s: host shadows of the scene are inconsistent", what);
        std::vector<uint32_t> islot;
        const sbq::Defect d = sbq::invert_slots(e->h_pslot.data(), e->P, islot);
        if (d != sbq::OK) SB_FAIL(e, SB_ERR_STATE, "%s: %s", what, sbq::defect_text(d));
        SB_TRY(s.buf[SBQ_B_ISLOT].grow(e, islot.size() * sizeof(uint32_t)));
        SB_HIP(e, hipMemcpyAsync(s.buf[SBQ_B_ISLOT].p, islot.data(), islot.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        SB_HIP(e, hipStreamSynchronize(e->stream)); // (the host vector goes out of scope)
        s.islot_valid = true;
        s.islot_ms = sbq_ms_since(t0);
    }
    if ((parts & SBQ_MATERIALS) && !s.mat_valid) { // sb_forces.hip: {spring, damp} per caller beam slot
        const auto t0 = std::chrono::steady_clock::now();
        if (e->h_beams.size() != e->B) SB_FAIL(e, SB_ERR_STATE, "%s: host shadows of the scene are inconsistent", what);
        std::vector<float> mat;
        const sbq::Defect d = sbq::beam_materials(e->h_user_slot.empty() ? nullptr : e->h_user_slot.data(), sb_user_beams(e), e->h_beams.data(), e->B, mat);
        if (d != sbq::OK) SB_FAIL(e, SB_ERR_STATE, "%s: %s", what, sbq::defect_text(d));
        SB_TRY(s.buf[SBQ_B_MAT].grow(e, mat.size() * sizeof(float)));
        SB_HIP(e, hipMemcpyAsync(s.buf[SBQ_B_MAT].p, mat.data(), mat.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
        SB_HIP(e, hipStreamSynchronize(e->stream)); // (the host vector goes out of scope)
        s.mat_valid = true;
        s.mat_ms = sbq_ms_since(t0);
    }
    return SB_OK;
}

sb_status sbq_user_slots(sb_engine *e, const char *what, std::vector<uint2> &slots)
{
    const uint32_t maxP = e->opt.max_particles, Bu = sb_user_beams(e);
    slots.resize(std::max<uint32_t>(Bu, 1));
    sbt::parallel_ranges(Bu, 1 << 16, [&](size_t u0, size_t u1) {
        for (size_t u = u0; u < u1; u++) slots[u] = make_uint2(sb_user_slot(e, u), map_get(e, e->h_mapping.data(), (size_t)maxP + u));
    });
    for (uint32_t u = 0; u < Bu; u++)
        if (slots[u].x >= e->B || slots[u].y >= e->opt.max_beams) SB_FAIL(e, SB_ERR_STATE, "%s: beam slot outside the scene", what);
    return SB_OK;
}

// ---------------------------------------------------------------- the exclusive scan

#define SBQ_WAVES (SBQ_BLOCK / 64u)

// the sum of the workgroup's values, and in *before the sum of the values of the threads below this one
template <class T>
SB_DEV T sbq_block_sum(T v, T *s_wave, T *before)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    T inc = v;
#pragma unroll
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const T u = __shfl_up(inc, off, 64);
        if (lane >= off) inc += u;
    }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    T base = inc - v, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < SBQ_WAVES; w++) {
        const T t = s_wave[w];
        base += w < wave ? t : (T)0;
        total += t;
    }
    __syncthreads(); // (s_wave may be written again)
    *before = base;
    return total;
}

template <class T>
__global__ __launch_bounds__(SBQ_BLOCK) void k_report_scan_reduce(const uint32_t *__restrict__ in, uint64_t n, T *__restrict__ bsum)
{
    __shared__ T s_wave[SBQ_WAVES];
    const uint64_t k0 = (uint64_t)blockIdx.x * SBQ_SCAN + threadIdx.x * SBQ_PER;
    T v = 0, before;
#pragma unroll
    for (uint32_t q = 0; q < SBQ_PER; q++)
        if (k0 + q < n) v += (T)in[k0 + q];
    const T total = sbq_block_sum(v, s_wave, &before);
    if (threadIdx.x == 0u) bsum[blockIdx.x] = total;
}

template <class T>
__global__ __launch_bounds__(SBQ_BLOCK) void k_report_scan_sums(T *bsum, uint32_t nb, T *total)
{
    __shared__ T s_wave[SBQ_WAVES];
    T carry = 0;
    for (uint32_t at = 0; at < nb; at += SBQ_BLOCK) { // (uniform)
        const uint32_t k = at + threadIdx.x;
        const T v = k < nb ? bsum[k] : (T)0;
        T before;
        const T sum = sbq_block_sum(v, s_wave, &before);
        if (k < nb) bsum[k] = carry + before;
        carry += sum;
    }
    if (total && threadIdx.x == 0u) *total = carry;
}

// (a thread reads its SBQ_PER words before it writes them and nobody else touches them: `out` may be `in`)
template <class T>
__global__ __launch_bounds__(SBQ_BLOCK) void k_report_scan_add(const uint32_t *in, uint64_t n, const T *__restrict__ bsum, T *out)
{
    __shared__ T s_wave[SBQ_WAVES];
    const uint64_t k0 = (uint64_t)blockIdx.x * SBQ_SCAN + threadIdx.x * SBQ_PER;
    uint32_t w[SBQ_PER];
    T v = 0, before;
#pragma unroll
    for (uint32_t q = 0; q < SBQ_PER; q++) {
        w[q] = k0 + q < n ? in[k0 + q] : 0u;
        v += (T)w[q];
    }
    (void)sbq_block_sum(v, s_wave, &before);
    T at = bsum[blockIdx.x] + before;
#pragma unroll
    for (uint32_t q = 0; q < SBQ_PER; q++) {
        if (k0 + q < n) out[k0 + q] = at;
        at += (T)w[q];
    }
}

template <class T>
void sbq_scan(sb_engine *e, const uint32_t *in, uint64_t n, T *bsum, T *out, T *total)
{
    const uint32_t nb = (uint32_t)((n + SBQ_SCAN - 1u) / SBQ_SCAN);
    k_report_scan_reduce<T><<<nb, SBQ_BLOCK, 0, e->stream>>>(in, n, bsum);
    k_report_scan_sums<T><<<1, SBQ_BLOCK, 0, e->stream>>>(bsum, nb, total);
    k_report_scan_add<T><<<nb, SBQ_BLOCK, 0, e->stream>>>(in, n, bsum, out);
}
template void sbq_scan<uint32_t>(sb_engine *, const uint32_t *, uint64_t, uint32_t *, uint32_t *, uint32_t *);
template void sbq_scan<unsigned long long>(sb_engine *, const uint32_t *, uint64_t, unsigned long long *, unsigned long long *, unsigned long long *);

std::vector<const void *> sbq_scan_kernels(bool wide)
{
    std::vector<const void *> ks = {(const void *)k_report_scan_reduce<uint32_t>, (const void *)k_report_scan_sums<uint32_t>,
                                    (const void *)k_report_scan_add<uint32_t>};
    if (wide)
        ks.insert(ks.end(), {(const void *)k_report_scan_reduce<unsigned long long>, (const void *)k_report_scan_sums<unsigned long long>,
                             (const void *)k_report_scan_add<unsigned long long>});
    return ks;
}
