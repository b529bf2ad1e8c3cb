/*
 * c_abi_nearest.c -- a hover test over a whole engine from plain C (C99): sb_nearest of include/softbody.h.
 *
 * Builds the reference's default scene (main.ts:188-246: seven lattice blobs and two free particles, 119 particles / 299 beams) in
 * the wide v2 byte layout by hand and asks about a row of sixteen cursor positions across it: what is nearest within 60 -- a
 * particle, a beam or a wall --, where on it, and how much is within reach?  Then the same positions for particles only, without a
 * limit.  Build and run (tests/test_c_nearest_example.py does exactly this):
 *   gcc -std=c99 -Iinclude examples/c_abi_nearest.c -o c_abi_nearest \
 *       -Lsoftbody-webgpu_amd/csrc -lsoftbody_hip -Wl,-rpath,$PWD/softbody-webgpu_amd/csrc -lm
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "softbody.h"

#define MAXP 128
#define MAXB 320
#define POINTS 16

static float particles[MAXP * 6];
static unsigned char beams[MAXB * SB_BEAM_STRIDE_V2];
static unsigned int mapping[MAXP + MAXB];
static unsigned int np, nb;

static void add_beam(unsigned int a, unsigned int b, float length, float spring, float damp, float yield, float limit)
{
    unsigned int ends[2] = {a, b};
    float f[9] = {length, length, length, spring, damp, yield, limit, 0.0f, 0.0f};
    memcpy(beams + (size_t)nb * SB_BEAM_STRIDE_V2, ends, 8);
    memcpy(beams + (size_t)nb * SB_BEAM_STRIDE_V2 + 8, f, sizeof f);
    mapping[MAXP + nb] = nb;
    nb++;
}

/* addRectangle, main.ts:203-214: w x h particles d apart, index = x * h + y; per particle the beams +y, +x, (+x, +y), (+x, -y) */
static void add_rectangle(double ox, double oy, double d, unsigned int w, unsigned int h, float spring, float damp, float yield, float limit)
{
    const unsigned int base = np;
    const float diag = (float)(sqrt(2.0) * d);
    for (unsigned int x = 0; x < w; x++)
        for (unsigned int y = 0; y < h; y++) {
            const unsigned int i = base + x * h + y;
            particles[6 * i] = (float)(x * d + ox);
            particles[6 * i + 1] = (float)(y * d + oy);
            mapping[i] = i;
            if (y + 1 < h) add_beam(i, i + 1, (float)d, spring, damp, yield, limit);
            if (x + 1 < w) add_beam(i, i + h, (float)d, spring, damp, yield, limit);
            if (y + 1 < h && x + 1 < w) add_beam(i, i + h + 1, diag, spring, damp, yield, limit);
            if (y > 0 && x + 1 < w) add_beam(i, i + h - 1, diag, spring, damp, yield, limit);
        }
    np += w * h;
}

static void add_free(float x, float y)
{
    particles[6 * np] = x;
    particles[6 * np + 1] = y;
    mapping[np] = np;
    np++;
}

int main(void)
{
    sb_options o;
    sb_default_options(&o);
    o.max_particles = MAXP;
    o.max_beams = MAXB;
    o.layout = SB_LAYOUT_V2;
    o.collision_mode = SB_COLLIDE_OFF;
    sb_engine *e = NULL;
    if (sb_create(&o, &e) != SB_OK) {
        fprintf(stderr, "sb_create: %s (there is no CPU fallback)\n", sb_last_error(NULL));
        return 2;
    }
    add_rectangle(185, 10, 60, 2, 2, 1.0f, 50.0f, 1.0f, 2.5f);
    add_rectangle(35, 10, 60, 2, 2, 1.0f, 50.0f, 1.0f, 2.5f);
    add_rectangle(20, 120, 30, 9, 4, 50.0f, 700.0f, 0.2f, 0.5f);
    add_free(445.0f, 10.0f);
    add_free(925.0f, 10.0f);
    add_rectangle(400, 40, 30, 20, 2, 500.0f, 800.0f, 0.1f, 0.5f);
    add_rectangle(700, 400, 40, 5, 5, 3.0f, 50.0f, 2.0f, 5.0f);
    add_rectangle(20, 900, 50, 2, 2, 0.05f, 10.0f, 2.0f, 3.0f);
    add_rectangle(20, 700, 50, 2, 2, 0.1f, 10.0f, 2.0f, 3.0f);
    unsigned char metadata[SB_METADATA_BYTES] = {0};
    unsigned int *mdu = (unsigned int *)metadata;
    float *mdf = (float *)metadata;
    mdu[0] = 3; mdu[1] = np;           /* particle vertex count, particle instance count */
    mdu[5] = 2; mdu[6] = nb;           /* beam vertex count, beam instance count */
    mdu[10] = MAXP; mdu[11] = MAXB;
    mdf[12] = 0.0f; mdf[13] = -0.5f;   /* gravity */
    mdf[14] = 0.5f; mdf[15] = 0.2f; mdf[16] = 0.5f; mdf[17] = 0.1f; mdf[18] = 0.001f; mdf[19] = 2.0f;
    mdf[20] = 1.0f;                    /* user strength */
    static sb_batch_near_point points[2 * POINTS];
    static float d[2 * POINTS], point[2 * POINTS][2];
    static int32_t hit[2 * POINTS][SB_BATCH_NEAR_HIT_WORDS], within[2 * POINTS][2];
    int64_t counts[SB_NEAREST_COUNT_WORDS];
    for (unsigned int j = 0; j < 2 * POINTS; j++) {
        memset(&points[j], 0, sizeof points[j]);
        points[j].mask = j < POINTS ? (SB_NEAR_PARTICLES | SB_NEAR_BEAMS | SB_NEAR_WALLS) : SB_NEAR_PARTICLES;
        points[j].px = 15.0f + 62.5f * (float)(j % POINTS);
        points[j].py = 75.0f + 20.0f * (float)(j % POINTS);
        points[j].rmax = j < POINTS ? 60.0f : INFINITY;
        points[j].skip_label = -1;
    }
    if (sb_write_buffers(e, metadata, sizeof metadata, mapping, sizeof mapping, particles, sizeof particles, beams, sizeof beams) != SB_OK ||
        sb_nearest(e, NULL, points, 2 * POINTS, NULL, d, &hit[0][0], &point[0][0], &within[0][0], counts) != SB_OK) {
        fprintf(stderr, "engine call failed: %s\n", sb_last_error(e));
        return 3;
    }
    static const char *kinds[4] = {"nothing", "particle", "beam", "wall"};
    int ok = np == 119 && nb == 299 && counts[0] == 2 * POINTS && counts[1] >= POINTS && counts[7] == 0;
    for (unsigned int j = 0; j < 2 * POINTS; j++) {
        uint32_t bits;
        memcpy(&bits, &d[j], 4);
        ok = ok && hit[j][0] >= 0 && hit[j][0] <= 3 && (j < POINTS || (hit[j][0] == SB_BATCH_NEAR_PARTICLE && within[j][0] == 119 && within[j][1] == 0));
        printf("pass %u point %2u: distance %.3f (bits %08x) to %s %d at (%.3f, %.3f), within reach %d particles %d beams\n", j / POINTS, j % POINTS, (double)d[j],
               (unsigned)bits, kinds[hit[j][0] & 3], (int)hit[j][1], (double)point[j][0], (double)point[j][1], (int)within[j][0], (int)within[j][1]);
    }
    printf("counts: valid %lld, particles %lld, beams %lld, walls %lld, swept %lld, outside %lld, long %lld\n", (long long)counts[0], (long long)counts[1],
           (long long)counts[2], (long long)counts[3], (long long)counts[4], (long long)counts[5], (long long)counts[6]);
    sb_destroy(e);
    puts(ok ? "C_ABI_NEAREST_OK" : "C_ABI_NEAREST_UNEXPECTED");
    return ok ? 0 : 1;
}
