/*
 * c_abi_cut.c -- cutting beams on the GPU from plain C (C99): sb_cut of include/softbody.h.
 *
 * Builds the reference's default scene (main.ts:188-246: seven lattice blobs and two free particles, 119 particles / 299 beams) in
 * the wide v2 byte layout by hand, cuts it with ONE knife stroke from (685, 0) to (685, 1000) -- the line between columns 9 and 10
 * of the long 20 x 2 strip, which no other blob reaches -- runs a frame, whose delete pass removes the beams the stroke crossed,
 * and prints the counts of sb_bodies before and after: the strip is in two, so there is one body more.  Build and run
 * (tests/test_c_cut_example.py does exactly this):
 *   gcc -std=c99 -Iinclude examples/c_abi_cut.c -o c_abi_cut \
 *       -Lsoftbody-webgpu_amd/csrc -lsoftbody_hip -Wl,-rpath,$PWD/softbody-webgpu_amd/csrc -lm
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "softbody.h"

#define MAXP 128
#define MAXB 320

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
        fprintf(stderr, "sb_create: %s\n", sb_last_error(NULL));
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
    sb_cut_shape knife;
    memset(&knife, 0, sizeof knife);
    knife.kind = SB_CUT_SEGMENT;
    knife.x0 = 685.0f; knife.y0 = 0.0f; knife.x1 = 685.0f; knife.y1 = 1000.0f;
    static uint8_t hit[MAXB];
    int64_t before[SB_BODY_WORDS], pending[SB_BODY_WORDS], after[SB_BODY_WORDS], counts[SB_CUT_COUNT_WORDS];
    static int32_t labels[MAXP];
    if (sb_write_buffers(e, metadata, sizeof metadata, mapping, sizeof mapping, particles, sizeof particles, beams, sizeof beams) != SB_OK ||
        sb_bodies(e, NULL, labels, NULL, before) != SB_OK ||
        sb_cut(e, NULL, &knife, 1, hit, counts) != SB_OK ||
        sb_bodies(e, NULL, labels, NULL, pending) != SB_OK ||   /* a pending flag still connects */
        sb_frame(e) != SB_OK ||
        sb_bodies(e, NULL, labels, NULL, after) != SB_OK) {
        fprintf(stderr, "engine call failed: %s\n", sb_last_error(e));
        return 3;
    }
    unsigned int marked = 0;
    for (unsigned int d = 0; d < nb; d++) marked += hit[d];
    printf("scene: %u particles, %u beams\n", np, nb);
    printf("cut: tested %lld, hit %lld, flagged %lld, already flagged %lld\n", (long long)counts[0], (long long)counts[1],
           (long long)counts[2], (long long)counts[3]);
    printf("bodies before the cut: %lld (largest %lld particles)\n", (long long)before[0], (long long)before[1]);
    printf("bodies with the cut pending: %lld\n", (long long)pending[0]);
    printf("bodies after the frame: %lld (largest %lld particles)\n", (long long)after[0], (long long)after[1]);
    /* the stroke crosses the strip's two +x beams and two diagonals between columns 9 and 10, and nothing else */
    int ok = np == 119 && nb == 299 && counts[0] == 299 && counts[1] == 4 && counts[2] == 4 && counts[3] == 0 && marked == 4 &&
             pending[0] == before[0] && after[0] == before[0] + 1;
    sb_destroy(e);
    puts(ok ? "C_ABI_CUT_OK" : "C_ABI_CUT_UNEXPECTED");
    return ok ? 0 : 1;
}
