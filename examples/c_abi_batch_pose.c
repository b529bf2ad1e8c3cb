/*
 * c_abi_batch_pose.c -- the pose of a body against its reset state on the GPU from plain C (C99): sb_batch_pose_device of
 * include/softbody.h.
 *
 * A 3 x 3 lattice of spacing 10 at integer coordinates (no beams: the labels put all nine particles into group 0) is uploaded,
 * which also makes it the reset state; then its particles are turned by a quarter turn about the lattice's centre and shifted,
 * through sb_batch_write_particles_device.  Against the reset state (device_ref_f32 = NULL) the fit must find a = 0 and
 * b = I = I0 = 12 * 100 = 1200 exactly: every coordinate is a small integer.  It prints a, b and I.  The calls take device memory;
 * the HIP runtime functions this needs are looked up in the runtime the library has already loaded, so the file stays plain C
 * and links against the library alone.  Build and run (tests/test_c_batch_pose_example.py does exactly this):
 *   gcc -std=c99 -Iinclude examples/c_abi_batch_pose.c -o c_abi_batch_pose \
 *       -Lsoftbody-webgpu_amd/csrc -lsoftbody_hip -Wl,-rpath,$PWD/softbody-webgpu_amd/csrc -lm -ldl
 */
#define _GNU_SOURCE /* RTLD_DEFAULT */
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "softbody.h"

#define MAXP 16
#define MAXB 8
#define NP 9

typedef int (*hip_malloc_fn)(void **, size_t);
typedef int (*hip_memcpy_fn)(void *, const void *, size_t, int);
typedef int (*hip_free_fn)(void *);
#define HIP_HOST_TO_DEVICE 1
#define HIP_DEVICE_TO_HOST 2

int main(void)
{
    static float particles[MAXP * 6], turned[MAXP * 6];
    static unsigned char beams[MAXB * SB_BEAM_STRIDE_V1];
    static unsigned short mapping[MAXP + MAXB];
    static int32_t labels[MAXP];
    for (int i = 0; i < NP; i++) {
        const float x = 100.0f + 10.0f * (float)(i % 3), y = 200.0f + 10.0f * (float)(i / 3);
        particles[6 * i] = x, particles[6 * i + 1] = y;
        /* a quarter turn about the centre (110, 210): (dx, dy) -> (-dy, dx); then a shift by (50, -20) */
        turned[6 * i] = 110.0f - (y - 210.0f) + 50.0f, turned[6 * i + 1] = 210.0f + (x - 110.0f) - 20.0f;
        mapping[i] = (unsigned short)i;
    }
    for (int i = 0; i < MAXP; i++) labels[i] = i < NP ? 0 : -1;

    unsigned char metadata[SB_METADATA_BYTES] = {0};
    unsigned int mdu[28] = {0};
    float mdf[28] = {0};
    mdu[0] = 3; mdu[1] = NP;                 /* particle vertex count, particle instance count (engineMapping.ts:252-273) */
    mdu[5] = 2; mdu[6] = 0;                  /* beam vertex count, beam instance count */
    mdu[10] = MAXP; mdu[11] = MAXB;
    memcpy(metadata, mdu, sizeof metadata);
    mdf[12] = 0.0f; mdf[13] = -0.5f;         /* gravity; border elasticity, border friction, elasticity, friction, drag (:264-272) */
    mdf[14] = 0.5f; mdf[15] = 0.2f; mdf[16] = 0.5f; mdf[17] = 0.1f; mdf[18] = 0.001f; mdf[19] = 2.0f;
    mdf[20] = 1.0f;                          /* user strength */
    memcpy(metadata + 48, mdf + 12, 9 * sizeof(float));

    sb_batch_options o;
    sb_batch_default_options(&o);
    o.n_scenes = 1;
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
    static float row[SB_BATCH_POSE_WORDS];
    static double m[SB_BATCH_POSE_MOMENT_WORDS];
    void *d_part = NULL, *d_labels = NULL, *d_row = NULL, *d_m = NULL;
    if (hip_malloc(&d_part, sizeof turned) || hip_malloc(&d_labels, sizeof labels) || hip_malloc(&d_row, sizeof row) || hip_malloc(&d_m, sizeof m) ||
        hip_memcpy(d_part, turned, sizeof turned, HIP_HOST_TO_DEVICE) || hip_memcpy(d_labels, labels, sizeof labels, HIP_HOST_TO_DEVICE)) {
        fprintf(stderr, "hipMalloc / hipMemcpy failed\n");
        return 3;
    }
    if (sb_batch_write_scene(b, 0, 1, metadata, sizeof metadata, mapping, sizeof mapping, particles, sizeof particles, beams, sizeof beams) != SB_OK ||
        sb_batch_write_particles_device(b, d_part) != SB_OK || sb_batch_pose_device(b, d_labels, NULL, 1, d_row, d_m, NULL) != SB_OK ||
        sb_batch_sync(b) != SB_OK || hip_memcpy(row, d_row, sizeof row, HIP_DEVICE_TO_HOST) || hip_memcpy(m, d_m, sizeof m, HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "batch call failed: %s\n", sb_batch_last_error(b));
        return 3;
    }
    printf("particles %.9g, label %.9g, matched %.9g, unmatched %.9g\n", (double)row[0], (double)row[1], (double)row[2], (double)row[3]);
    printf("centroid %.9g %.9g, reference centroid %.9g %.9g\n", (double)row[4], (double)row[5], (double)row[6], (double)row[7]);
    printf("a %.17g, b %.17g, I %.17g\n", m[0], m[1], m[2]);
    int ok = row[0] == 9.0f && row[1] == 0.0f && row[2] == 9.0f && row[3] == 0.0f && row[4] == 160.0f && row[5] == 190.0f && row[6] == 110.0f &&
             row[7] == 210.0f && m[0] == 0.0 && m[1] == 1200.0 && m[2] == 1200.0 && m[3] == 1200.0 && m[4] == 0.0 && m[5] == 9.0 && row[16] == 1.0f;
    hip_free(d_part), hip_free(d_labels), hip_free(d_row), hip_free(d_m);
    sb_batch_destroy(b);
    puts(ok ? "C_ABI_BATCH_POSE_OK" : "C_ABI_BATCH_POSE_UNEXPECTED");
    return ok ? 0 : 1;
}
