/*
 * c_abi_batch_graph.c -- the beam graph of a batch on the GPU from plain C (C99): sb_batch_graph_device of include/softbody.h.
 *
 * Builds the reference's default scene (main.ts:188-246: 119 particles / 299 beams) by hand, uploads it into both scenes of a
 * batch of two and prints the graph's counts: listed beams, particles of degree >= 1, the largest degree and who has it.  Then it
 * welds the scene's two free particles (data indices 44 and 45, both of degree 0) in scene 0 with one row of
 * sb_batch_add_beams_device and asks again: one beam and two connected particles more in scene 0, whose new edge reads {44, 45}
 * in `ends` and is the one row of each of the two particles in `nbr`; scene 1 as it was.  The calls take device memory; the three
 * HIP runtime functions this needs are looked up in the runtime the library has already loaded, so the file stays plain C and
 * links against the library alone.  Build and run (tests/test_c_batch_graph_example.py does exactly this):
 *   gcc -std=c99 -Iinclude examples/c_abi_batch_graph.c -o c_abi_batch_graph \
 *       -Lsoftbody-webgpu_amd/csrc -lsoftbody_hip -Wl,-rpath,$PWD/softbody-webgpu_amd/csrc -lm -ldl
 */
#define _GNU_SOURCE /* RTLD_DEFAULT */
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "softbody.h"

#define MAXP 128
#define MAXB 320
#define NS 2

static float particles[MAXP * 6];
static unsigned char beams[MAXB * SB_BEAM_STRIDE_V1];
static unsigned short mapping[MAXP + MAXB];
static unsigned P, B;

static void add_beam(unsigned a, unsigned b, double len, float spring, float damp, float yield, float limit)
{
    unsigned short ends[2] = {(unsigned short)a, (unsigned short)b};
    float f[9] = {(float)len, (float)len, (float)len, spring, damp, yield, limit, 0.0f, 0.0f};
    memcpy(beams + (size_t)B * SB_BEAM_STRIDE_V1, ends, 4);
    memcpy(beams + (size_t)B * SB_BEAM_STRIDE_V1 + 4, f, sizeof f);
    B++;
}

/* addRectangle (main.ts:203-214): particle (x, y) at (ox + x d, oy + y d), data index base + x h + y; per particle the beams
 * to +y, +x, the diagonal and the anti-diagonal where they exist */
static void rectangle(double ox, double oy, double d, unsigned w, unsigned h, float spring, float damp, float yield, float limit)
{
    const unsigned base = P;
    for (unsigned x = 0; x < w; x++)
        for (unsigned y = 0; y < h; y++) {
            const unsigned i = base + x * h + y;
            particles[i * 6 + 0] = (float)(x * d + ox);
            particles[i * 6 + 1] = (float)(y * d + oy);
            if (y < h - 1) add_beam(i, i + 1, d, spring, damp, yield, limit);
            if (x < w - 1) add_beam(i, i + h, d, spring, damp, yield, limit);
            if (y < h - 1 && x < w - 1) add_beam(i, i + h + 1, sqrt(2.0) * d, spring, damp, yield, limit);
            if (y > 0 && x < w - 1) add_beam(i, i + h - 1, sqrt(2.0) * d, spring, damp, yield, limit);
        }
    P += w * h;
}

static void free_particle(double x, double y)
{
    particles[P * 6 + 0] = (float)x;
    particles[P * 6 + 1] = (float)y;
    P++;
}

typedef int (*hip_malloc_fn)(void **, size_t);
typedef int (*hip_memcpy_fn)(void *, const void *, size_t, int);
typedef int (*hip_free_fn)(void *);
#define HIP_HOST_TO_DEVICE 1
#define HIP_DEVICE_TO_HOST 2

int main(void)
{
    rectangle(185, 10, 60, 2, 2, 1, 50, 1, 2.5f);       /* main.ts:218 */
    rectangle(35, 10, 60, 2, 2, 1, 50, 1, 2.5f);        /* :219 */
    rectangle(20, 120, 30, 9, 4, 50, 700, 0.2f, 0.5f);  /* :220 */
    free_particle(445, 10);                             /* :221 */
    free_particle(925, 10);                             /* :222 */
    rectangle(400, 40, 30, 20, 2, 500, 800, 0.1f, 0.5f); /* :223 */
    rectangle(700, 400, 40, 5, 5, 3, 50, 2, 5);         /* :224 */
    rectangle(20, 900, 50, 2, 2, 0.05f, 10, 2, 3);      /* :240 */
    rectangle(20, 700, 50, 2, 2, 0.1f, 10, 2, 3);       /* :241 */
    for (unsigned s = 0; s < P; s++) mapping[s] = (unsigned short)s;
    for (unsigned s = 0; s < B; s++) mapping[MAXP + s] = (unsigned short)s;

    unsigned char metadata[SB_METADATA_BYTES] = {0};
    unsigned int mdu[28] = {0};
    float mdf[28] = {0};
    mdu[0] = 3; mdu[1] = P;                  /* particle vertex count, particle instance count (engineMapping.ts:252-273) */
    mdu[5] = 2; mdu[6] = B;                  /* beam vertex count, beam instance count */
    mdu[10] = MAXP; mdu[11] = MAXB;
    memcpy(metadata, mdu, sizeof metadata);
    mdf[12] = 0.0f; mdf[13] = -0.5f;         /* gravity; border elasticity, border friction, elasticity, friction, drag (:264-272) */
    mdf[14] = 0.5f; mdf[15] = 0.2f; mdf[16] = 0.5f; mdf[17] = 0.1f; mdf[18] = 0.001f; mdf[19] = 2.0f;
    mdf[20] = 1.0f;                          /* user strength */
    memcpy(metadata + 48, mdf + 12, 9 * sizeof(float));

    sb_batch_options o;
    sb_batch_default_options(&o);
    o.n_scenes = NS;
    o.max_particles = MAXP;
    o.max_beams = MAXB;
    sb_batch *b = NULL;
    if (sb_batch_create(&o, &b) != SB_OK) {
        fprintf(stderr, "sb_batch_create: %s\n", sb_batch_last_error(NULL));
        return 2;
    }
    /* the HIP runtime is in the process now: the library brought it */
    hip_malloc_fn hip_malloc;
    hip_memcpy_fn hip_memcpy;
    hip_free_fn hip_free;
    void *sym[3] = {dlsym(RTLD_DEFAULT, "hipMalloc"), dlsym(RTLD_DEFAULT, "hipMemcpy"), dlsym(RTLD_DEFAULT, "hipFree")};
    memcpy(&hip_malloc, &sym[0], sizeof sym[0]);
    memcpy(&hip_memcpy, &sym[1], sizeof sym[1]);
    memcpy(&hip_free, &sym[2], sizeof sym[2]);
    if (!hip_malloc || !hip_memcpy || !hip_free) {
        fprintf(stderr, "the HIP runtime's hipMalloc / hipMemcpy / hipFree were not found\n");
        return 3;
    }
    static int32_t ends[NS][MAXB][2], row_ptr[NS][MAXP + 1], nbr[NS][2 * MAXB][2];
    int32_t before[NS][SB_BATCH_GRAPH_COUNT_WORDS], after[NS][SB_BATCH_GRAPH_COUNT_WORDS], result[NS];
    sb_batch_new_beam rows[NS];
    void *d_ends = NULL, *d_row_ptr = NULL, *d_nbr = NULL, *d_counts = NULL, *d_rows = NULL, *d_result = NULL;
    if (hip_malloc(&d_ends, sizeof ends) || hip_malloc(&d_row_ptr, sizeof row_ptr) || hip_malloc(&d_nbr, sizeof nbr) ||
        hip_malloc(&d_counts, sizeof before) || hip_malloc(&d_rows, sizeof rows) || hip_malloc(&d_result, sizeof result)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 3;
    }
    if (sb_batch_write_scene(b, 0, NS, metadata, sizeof metadata, mapping, sizeof mapping, particles, sizeof particles, beams, sizeof beams) != SB_OK ||
        sb_batch_graph_device(b, 0, NULL, NULL, NULL, NULL, d_counts) != SB_OK || sb_batch_sync(b) != SB_OK ||
        hip_memcpy(before, d_counts, sizeof before, HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "batch call failed: %s\n", sb_batch_last_error(b));
        return 3;
    }
    /* weld the two free particles of scene 0 (rest length = their current distance); scene 1 gets an empty row */
    const int32_t wa = 44, wb = 45;
    memset(rows, 0, sizeof rows);
    rows[0].a = wa, rows[0].b = wb;
    rows[0].spring = 50.0f, rows[0].damp = 700.0f, rows[0].yield_strain = 0.2f, rows[0].strain_break_limit = 0.5f;
    rows[1].a = SB_BATCH_ADD_EMPTY;
    if (hip_memcpy(d_rows, rows, sizeof rows, HIP_HOST_TO_DEVICE) ||
        sb_batch_add_beams_device(b, SB_BATCH_ADD_LENGTH_CURRENT, d_rows, 1, d_result, NULL) != SB_OK ||
        sb_batch_graph_device(b, 0, d_ends, NULL, d_row_ptr, d_nbr, d_counts) != SB_OK || sb_batch_sync(b) != SB_OK ||
        hip_memcpy(result, d_result, sizeof result, HIP_DEVICE_TO_HOST) || hip_memcpy(after, d_counts, sizeof after, HIP_DEVICE_TO_HOST) ||
        hip_memcpy(ends, d_ends, sizeof ends, HIP_DEVICE_TO_HOST) || hip_memcpy(row_ptr, d_row_ptr, sizeof row_ptr, HIP_DEVICE_TO_HOST) ||
        hip_memcpy(nbr, d_nbr, sizeof nbr, HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "batch call failed: %s\n", sb_batch_last_error(b));
        return 3;
    }
    printf("scene: %u particles, %u beams, in %d scenes\n", P, B, NS);
    for (int s = 0; s < NS; s++) {
        printf("scene %d before: beams %d, connected particles %d, largest degree %d at particle %d\n", s, before[s][0], before[s][1], before[s][2],
               before[s][3]);
        printf("scene %d after:  beams %d, connected particles %d, largest degree %d at particle %d\n", s, after[s][0], after[s][1], after[s][2],
               after[s][3]);
    }
    const int32_t d = result[0], ra = row_ptr[0][wa], rb = row_ptr[0][wb];
    int ok = P == 119 && B == 299 && d == (int32_t)B && result[1] == SB_BATCH_ADD_EMPTY;
    if (ok) {
        printf("the weld: beam %d joins {%d, %d}; particle %d's rows %d .. %d: {%d, %d}; particle %d's rows %d .. %d: {%d, %d}\n", d, ends[0][d][0],
               ends[0][d][1], wa, ra, row_ptr[0][wa + 1] - 1, nbr[0][ra][0], nbr[0][ra][1], wb, rb, row_ptr[0][wb + 1] - 1, nbr[0][rb][0], nbr[0][rb][1]);
        ok = before[0][0] == 299 && after[0][0] == 300 && after[0][1] == before[0][1] + 2 && after[0][2] == before[0][2] && after[0][3] == before[0][3] &&
             memcmp(after[1], before[1], sizeof before[1]) == 0 && memcmp(before[0], before[1], sizeof before[1]) == 0 && ends[0][d][0] == wa &&
             ends[0][d][1] == wb && ends[1][d][0] == -1 && row_ptr[0][wa + 1] == ra + 1 && row_ptr[0][wb + 1] == rb + 1 && nbr[0][ra][0] == wb &&
             nbr[0][ra][1] == d && nbr[0][rb][0] == wa && nbr[0][rb][1] == d && row_ptr[0][MAXP] == 600 && row_ptr[1][MAXP] == 598 &&
             nbr[0][600][0] == -1 && nbr[1][598][1] == -1;
    }
    hip_free(d_ends), hip_free(d_row_ptr), hip_free(d_nbr), hip_free(d_counts), hip_free(d_rows), hip_free(d_result);
    sb_batch_destroy(b);
    puts(ok ? "C_ABI_BATCH_GRAPH_OK" : "C_ABI_BATCH_GRAPH_UNEXPECTED");
    return ok ? 0 : 1;
}
