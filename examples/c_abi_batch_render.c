/*
 * c_abi_batch_render.c -- a picture of one scene of a batch from plain C (C99): four copies of the web app's default scene
 * (main.ts:218-241, built as in c_abi_render.c) in one sb_batch, one frame on the GPU for all of them in one launch, then
 * sb_batch_render_scene of scene 0 into host memory and a binary PPM on disk -- the file host/render.js renderPPM writes for
 * the same state.  Build and run (tests/test_c_batch_render_example.py does exactly this):
 *   gcc -std=c99 -Iinclude examples/c_abi_batch_render.c -o c_abi_batch_render -lm \
 *       -Lsoftbody-webgpu_amd/csrc -lsoftbody_hip -Wl,-rpath,$PWD/softbody-webgpu_amd/csrc
 *   ./c_abi_batch_render out.ppm [resolution]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "softbody.h"

#define MAXP 256
#define MAXB 512

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

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s out.ppm [resolution]\n", argv[0]);
        return 1;
    }
    const unsigned res = argc > 2 ? (unsigned)strtoul(argv[2], NULL, 10) : 64u;
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
    o.n_scenes = 4;
    o.max_particles = MAXP;
    o.max_beams = MAXB;
    sb_batch *b = NULL;
    if (sb_batch_create(&o, &b) != SB_OK) {
        fprintf(stderr, "sb_batch_create: %s\n", sb_batch_last_error(NULL));
        return 2;
    }
    size_t bytes = (size_t)res * res * 3;
    unsigned char *rgb = malloc(bytes ? bytes : 1);
    sb_batch_render_options ro;
    memset(&ro, 0, sizeof ro);
    ro.struct_size = sizeof ro;
    ro.resolution = res; /* bounds and radius: the batch's (1000, 10) */
    if (!rgb || sb_batch_write_scene(b, 0, o.n_scenes, metadata, sizeof metadata, mapping, sizeof mapping, particles, sizeof particles,
                                     beams, sizeof beams) != SB_OK ||
        sb_batch_frame(b, 1) != SB_OK || sb_batch_render_scene(b, 0, &ro, rgb, bytes) != SB_OK) {
        fprintf(stderr, "batch call failed: %s\n", sb_batch_last_error(b));
        return 3;
    }
    sb_batch_destroy(b);
    FILE *f = fopen(argv[1], "wb");
    if (!f || fprintf(f, "P6\n%u %u\n255\n", res, res) < 0 || fwrite(rgb, 1, bytes, f) != bytes || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[1]);
        return 4;
    }
    free(rgb);
    printf("C_BATCH_RENDER_OK %u scenes of %u particles, %u beams, %ux%u -> %s\n", o.n_scenes, P, B, res, res, argv[1]);
    return 0;
}
