/*
 * c_abi_batch_spawn.c -- spawning a body on the GPU from plain C (C99): sb_batch_add_particles_device and
 * sb_batch_add_beams_device of include/softbody.h.
 *
 * Builds the reference's default scene (main.ts:188-246: 119 particles / 299 beams) by hand, uploads it into both scenes of a
 * batch of two, and spawns a triangle into scene 0: three particles in one call (scene 1 gets empty rows), then three beams
 * between the data indices that call returned.  One frame is stepped and the bodies are counted before and after: one more in
 * scene 0, unchanged in scene 1.  The calls take device memory; the three HIP runtime functions this needs are looked up in the
 * runtime the library has already loaded, so the file stays plain C and links against the library alone.  Build and run
 * (tests/test_c_batch_spawn_example.py does exactly this):
 *   gcc -std=c99 -Iinclude examples/c_abi_batch_spawn.c -o c_abi_batch_spawn \
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
    int32_t before[NS][SB_BATCH_BODY_WORDS], after[NS][SB_BATCH_BODY_WORDS], result[NS][3], counts[NS][SB_BATCH_SPAWN_COUNT_WORDS];
    int32_t beam_result[NS][3], beam_counts[NS][SB_BATCH_ADD_COUNT_WORDS];
    sb_batch_new_particle rows[NS][3];
    sb_batch_new_beam welds[NS][3];
    void *d_body = NULL, *d_rows = NULL, *d_result = NULL, *d_counts = NULL, *d_welds = NULL;
    if (hip_malloc(&d_body, sizeof before) || hip_malloc(&d_rows, sizeof rows) || hip_malloc(&d_result, sizeof result) ||
        hip_malloc(&d_counts, sizeof counts) || hip_malloc(&d_welds, sizeof welds)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 3;
    }
    /* a triangle of side 30 in the empty middle of the box, falling; scene 1: empty rows */
    const float corner[3][2] = {{500.0f, 500.0f}, {530.0f, 500.0f}, {515.0f, 526.0f}};
    memset(rows, 0, sizeof rows);
    for (int j = 0; j < 3; j++) {
        rows[0][j].x = corner[j][0], rows[0][j].y = corner[j][1], rows[0][j].vy = -2.0f;
        rows[1][j].tag = SB_BATCH_SPAWN_EMPTY;
    }
    if (sb_batch_write_scene(b, 0, NS, metadata, sizeof metadata, mapping, sizeof mapping, particles, sizeof particles, beams, sizeof beams) != SB_OK ||
        sb_batch_bodies_device(b, NULL, NULL, d_body) != SB_OK || hip_memcpy(d_rows, rows, sizeof rows, HIP_HOST_TO_DEVICE) ||
        sb_batch_add_particles_device(b, SB_BATCH_SPAWN_SKIP_TOUCHING, d_rows, 3, d_result, d_counts) != SB_OK || sb_batch_sync(b) != SB_OK ||
        hip_memcpy(before, d_body, sizeof before, HIP_DEVICE_TO_HOST) || hip_memcpy(result, d_result, sizeof result, HIP_DEVICE_TO_HOST) ||
        hip_memcpy(counts, d_counts, sizeof counts, HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "batch call failed: %s\n", sb_batch_last_error(b));
        return 3;
    }
    /* the three sides, between the data indices the spawn returned (a row whose endpoint was not added stays empty) */
    memset(welds, 0, sizeof welds);
    for (int s = 0; s < NS; s++)
        for (int j = 0; j < 3; j++) {
            const int32_t a = result[s][j], c = result[s][(j + 1) % 3];
            welds[s][j].a = (a >= 0 && c >= 0) ? a : SB_BATCH_ADD_EMPTY, welds[s][j].b = c;
            welds[s][j].spring = 50.0f, welds[s][j].damp = 700.0f, welds[s][j].yield_strain = 0.2f, welds[s][j].strain_break_limit = 0.5f;
        }
    if (hip_memcpy(d_welds, welds, sizeof welds, HIP_HOST_TO_DEVICE) ||
        sb_batch_add_beams_device(b, SB_BATCH_ADD_LENGTH_CURRENT, d_welds, 3, d_result, d_counts) != SB_OK || sb_batch_frame(b, 1) != SB_OK ||
        sb_batch_bodies_device(b, NULL, NULL, d_body) != SB_OK || sb_batch_sync(b) != SB_OK ||
        hip_memcpy(beam_result, d_result, sizeof beam_result, HIP_DEVICE_TO_HOST) ||
        hip_memcpy(beam_counts, d_counts, sizeof beam_counts, HIP_DEVICE_TO_HOST) || hip_memcpy(after, d_body, sizeof after, HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "batch call failed: %s\n", sb_batch_last_error(b));
        return 3;
    }
    printf("scene: %u particles, %u beams, in %d scenes\n", P, B, NS);
    for (int s = 0; s < NS; s++)
        printf("scene %d: bodies before %d, after %d; particles %d %d %d (added %d, invalid %d, blocked %d, full %d); beams %d %d %d (added %d)\n", s,
               before[s][0], after[s][0], result[s][0], result[s][1], result[s][2], counts[s][0], counts[s][1], counts[s][2], counts[s][3],
               beam_result[s][0], beam_result[s][1], beam_result[s][2], beam_counts[s][0]);
    int ok = P == 119 && B == 299 && after[0][0] == before[0][0] + 1 && after[1][0] == before[1][0] && result[0][0] == (int32_t)P &&
             result[0][2] == (int32_t)P + 2 && result[1][0] == SB_BATCH_SPAWN_EMPTY && counts[0][0] == 3 && counts[1][0] == 0 &&
             beam_result[0][0] == (int32_t)B && beam_counts[0][0] == 3 && beam_counts[1][0] == 0;
    hip_free(d_body), hip_free(d_rows), hip_free(d_result), hip_free(d_counts), hip_free(d_welds);
    sb_batch_destroy(b);
    puts(ok ? "C_ABI_BATCH_SPAWN_OK" : "C_ABI_BATCH_SPAWN_UNEXPECTED");
    return ok ? 0 : 1;
}
