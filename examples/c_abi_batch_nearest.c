/*
 * c_abi_batch_nearest.c -- proximity queries of a batch on the GPU from plain C (C99): sb_batch_nearest_device of include/softbody.h.
 *
 * Builds the reference's default scene (main.ts:188-246: 119 particles / 299 beams) by hand, uploads it into both scenes of a
 * batch of two and asks about a grid of sixteen probe points in each: (100 + 250 i, 50 + 150 j), reach 120.  Scene 1's rows look at
 * particles and walls only.  It prints, per point, the distance (and its bits), what is nearest, its index, the closest point on it
 * and how many particles and beams lie within reach, then the counts of both scenes.  The calls take device memory; the three HIP
 * runtime functions this needs are looked up in the runtime the library has already loaded, so the file stays plain C and links
 * against the library alone.  Build and run (tests/test_c_batch_nearest_example.py does exactly this):
 *   gcc -std=c99 -Iinclude examples/c_abi_batch_nearest.c -o c_abi_batch_nearest \
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
#define POINTS 16

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
    static sb_batch_near_point points[NS][POINTS];
    static float d[NS][POINTS], q[NS][POINTS][2];
    static int32_t hit[NS][POINTS][SB_BATCH_NEAR_HIT_WORDS], within[NS][POINTS][2], counts[NS][SB_BATCH_NEAR_COUNT_WORDS];
    memset(points, 0, sizeof points); /* (the reserved words) */
    for (int s = 0; s < NS; s++)
        for (int j = 0; j < POINTS; j++) {
            points[s][j].mask = s == 0 ? SB_NEAR_PARTICLES | SB_NEAR_BEAMS | SB_NEAR_WALLS : SB_NEAR_PARTICLES | SB_NEAR_WALLS;
            points[s][j].px = 100.0f + 250.0f * (float)(j % 4), points[s][j].py = 50.0f + 150.0f * (float)(j / 4);
            points[s][j].rmax = 120.0f;
            points[s][j].skip_label = -1;
        }
    void *d_points = NULL, *d_d = NULL, *d_hit = NULL, *d_q = NULL, *d_within = NULL, *d_counts = NULL;
    if (hip_malloc(&d_points, sizeof points) || hip_malloc(&d_d, sizeof d) || hip_malloc(&d_hit, sizeof hit) || hip_malloc(&d_q, sizeof q) ||
        hip_malloc(&d_within, sizeof within) || hip_malloc(&d_counts, sizeof counts)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 3;
    }
    if (sb_batch_write_scene(b, 0, NS, metadata, sizeof metadata, mapping, sizeof mapping, particles, sizeof particles, beams, sizeof beams) != SB_OK ||
        hip_memcpy(d_points, points, sizeof points, HIP_HOST_TO_DEVICE) ||
        sb_batch_nearest_device(b, 0, d_points, POINTS, NULL, d_d, d_hit, d_q, d_within, d_counts) != SB_OK || sb_batch_sync(b) != SB_OK ||
        hip_memcpy(d, d_d, sizeof d, HIP_DEVICE_TO_HOST) || hip_memcpy(hit, d_hit, sizeof hit, HIP_DEVICE_TO_HOST) ||
        hip_memcpy(q, d_q, sizeof q, HIP_DEVICE_TO_HOST) || hip_memcpy(within, d_within, sizeof within, HIP_DEVICE_TO_HOST) ||
        hip_memcpy(counts, d_counts, sizeof counts, HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "batch call failed: %s\n", sb_batch_last_error(b));
        return 3;
    }
    static const char *kinds[4] = {"nothing", "particle", "beam", "wall"};
    printf("scene: %u particles, %u beams, in %d scenes; %d points, reach 120\n", P, B, NS, POINTS);
    int ok = P == 119 && B == 299;
    for (int s = 0; s < NS; s++) {
        for (int j = 0; j < POINTS; j++) {
            uint32_t bits;
            memcpy(&bits, &d[s][j], sizeof bits);
            const int kind = hit[s][j][0];
            ok = ok && kind >= SB_BATCH_NEAR_MISS && kind <= SB_BATCH_NEAR_WALL && hit[s][j][2] == -1 && (s == 0 || kind != SB_BATCH_NEAR_BEAM) &&
                 d[s][j] <= 120.0f && (s == 0 || within[s][j][1] == 0);
            printf("scene %d point %2d: distance %.9g (bits %08x) to %s %d at (%.9g, %.9g), within: %d particles, %d beams\n", s, j, (double)d[s][j], bits,
                   kinds[kind >= 0 && kind < 4 ? kind : 0], hit[s][j][1], (double)q[s][j][0], (double)q[s][j][1], within[s][j][0], within[s][j][1]);
        }
        printf("scene %d counts: valid %d, particles %d, beams %d, walls %d\n", s, counts[s][0], counts[s][1], counts[s][2], counts[s][3]);
        ok = ok && counts[s][0] == POINTS && counts[s][1] + counts[s][2] + counts[s][3] <= POINTS;
    }
    /* with the beams in the game nothing can be farther than without them, and the particles within reach are the same */
    for (int j = 0; j < POINTS; j++) ok = ok && d[0][j] <= d[1][j] && within[0][j][0] == within[1][j][0];
    ok = ok && counts[0][2] > 0 && counts[1][2] == 0;
    hip_free(d_points), hip_free(d_d), hip_free(d_hit), hip_free(d_q), hip_free(d_within), hip_free(d_counts);
    sb_batch_destroy(b);
    puts(ok ? "C_ABI_BATCH_NEAREST_OK" : "C_ABI_BATCH_NEAREST_UNEXPECTED");
    return ok ? 0 : 1;
}
