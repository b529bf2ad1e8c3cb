/*
 * c_abi_batch_forces.c -- beam and contact forces of a batch on the GPU from plain C (C99): sb_batch_forces_device of
 * include/softbody.h.
 *
 * Two particles 40 apart along x and one beam of rest length 30 between them (spring 2, damp 0.5, last_length 38): the beam is
 * stretched, force_mag = (30 - 40) * 2 + (38 - 40) * 0.5 = -21, and pulls each endpoint towards the other with 21.  It prints the
 * two rows, the tension and the counts.  The call takes device memory; the three HIP runtime functions this needs are looked up in
 * the runtime the library has already loaded, so the file stays plain C and links against the library alone.  Build and run
 * (tests/test_c_batch_forces_example.py does exactly this):
 *   gcc -std=c99 -Iinclude examples/c_abi_batch_forces.c -o c_abi_batch_forces \
 *       -Lsoftbody-webgpu_amd/csrc -lsoftbody_hip -Wl,-rpath,$PWD/softbody-webgpu_amd/csrc -lm -ldl
 */
#define _GNU_SOURCE /* RTLD_DEFAULT */
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "softbody.h"

#define MAXP 8
#define MAXB 8

typedef int (*hip_malloc_fn)(void **, size_t);
typedef int (*hip_memcpy_fn)(void *, const void *, size_t, int);
typedef int (*hip_free_fn)(void *);
#define HIP_DEVICE_TO_HOST 2

int main(void)
{
    static float particles[MAXP * 6];
    static unsigned char beams[MAXB * SB_BEAM_STRIDE_V1];
    static unsigned short mapping[MAXP + MAXB];
    particles[0] = 100.0f, particles[1] = 200.0f;
    particles[6] = 140.0f, particles[7] = 200.0f;
    const unsigned short ends[2] = {0, 1};
    /* length, target_length, last_length, spring, damp, yield_strain, strain_break_limit, strain, stress */
    const float f[9] = {30.0f, 30.0f, 38.0f, 2.0f, 0.5f, 5.0f, 50.0f, 0.0f, 0.0f};
    memcpy(beams, ends, 4);
    memcpy(beams + 4, f, sizeof f);
    mapping[0] = 0, mapping[1] = 1, mapping[MAXP] = 0;

    unsigned char metadata[SB_METADATA_BYTES] = {0};
    unsigned int mdu[28] = {0};
    float mdf[28] = {0};
    mdu[0] = 3; mdu[1] = 2;                  /* particle vertex count, particle instance count (engineMapping.ts:252-273) */
    mdu[5] = 2; mdu[6] = 1;                  /* beam vertex count, beam instance count */
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
    static float rows[MAXP][SB_BATCH_FORCE_WORDS], tension[MAXB];
    static int32_t counts[SB_BATCH_FORCE_COUNT_WORDS];
    void *d_rows = NULL, *d_tension = NULL, *d_counts = NULL;
    if (hip_malloc(&d_rows, sizeof rows) || hip_malloc(&d_tension, sizeof tension) || hip_malloc(&d_counts, sizeof counts)) {
        fprintf(stderr, "hipMalloc failed\n");
        return 3;
    }
    if (sb_batch_write_scene(b, 0, 1, metadata, sizeof metadata, mapping, sizeof mapping, particles, sizeof particles, beams, sizeof beams) != SB_OK ||
        sb_batch_forces_device(b, 0, NULL, d_rows, NULL, d_tension, d_counts) != SB_OK || sb_batch_sync(b) != SB_OK ||
        hip_memcpy(rows, d_rows, sizeof rows, HIP_DEVICE_TO_HOST) || hip_memcpy(tension, d_tension, sizeof tension, HIP_DEVICE_TO_HOST) ||
        hip_memcpy(counts, d_counts, sizeof counts, HIP_DEVICE_TO_HOST)) {
        fprintf(stderr, "batch call failed: %s\n", sb_batch_last_error(b));
        return 3;
    }
    for (int i = 0; i < 2; i++) {
        printf("particle %d:", i);
        for (unsigned k = 0; k < SB_BATCH_FORCE_WORDS; k++) printf(" %.9g", (double)rows[i][k]);
        printf("\n");
    }
    printf("tension of beam 0: %.9g\n", (double)tension[0]);
    printf("counts: particles %d, beams %d, touching %d, nonfinite %d\n", counts[0], counts[1], counts[2], counts[3]);
    int ok = rows[0][0] == 21.0f && rows[1][0] == -21.0f && tension[0] == -21.0f && counts[0] == 2 && counts[1] == 1 && counts[2] == 0 && counts[3] == 0;
    for (int i = 0; i < MAXP; i++)
        for (unsigned k = (i < 2 ? 1u : 0u); k < SB_BATCH_FORCE_WORDS; k++) ok = ok && rows[i][k] == 0.0f;
    hip_free(d_rows), hip_free(d_tension), hip_free(d_counts);
    sb_batch_destroy(b);
    puts(ok ? "C_ABI_BATCH_FORCES_OK" : "C_ABI_BATCH_FORCES_UNEXPECTED");
    return ok ? 0 : 1;
}
