// sb_batch_group_sort.h -- what the per-group reports of a batch (sb_batch_body_summary.hip, sb_batch_pose.hip) share
// besides sb_summary_math.h: the workgroup size, the bitonic network that sorts their keys in LDS, and the key that ranks the groups
// of a scene.  Device code; one workgroup of SBQ_BLOCK threads per scene.
#pragma once
#include "sb_batch.h"

// 256 threads as the sibling kernels: the sort's W / 2 = 512 compare-exchanges of the largest capacity are two per thread, and
// four waves keep a barrier (there are about 120 in a launch at W = 1024) cheap
#define SBQ_BLOCK 256u
#define SBQ_NONE 0xFFFFFFFFu
#define SBQ_LDS_DEFAULT_LIMIT (64u * 1024u) // above it a launch needs hipFuncAttributeMaxDynamicSharedMemorySize

static_assert(SB_BATCH_MAX_PARTICLES <= 1024 && SB_BATCH_MAX_BEAMS < 0x10000, "a rank key holds 10 bits of label, a count word 16 bits per count");

// ascending bitonic sort of a[0 .. W-1] (W a power of two) by the whole workgroup; ends in a barrier
SB_DEV void sbq_sort(uint32_t *a, uint32_t W, uint32_t tid)
{
    for (uint32_t k = 2u; k <= W; k <<= 1) {
        for (uint32_t j = k >> 1; j != 0u; j >>= 1) {
            for (uint32_t t = tid; t < (W >> 1); t += SBQ_BLOCK) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), p = i | j;
                const uint32_t x = a[i], y = a[p];
                if ((x > y) == ((i & k) == 0u)) a[i] = y, a[p] = x;
            }
            __syncthreads();
        }
    }
}

// the ranking: particles descending, then label ascending -- the ascending order of ~(particles << 10 | (1023 - label)); a group
// without particles has no key (SBQ_NONE sorts behind every key)
SB_DEV uint32_t sbq_rank_key(uint32_t particles, uint32_t label) { return particles ? ~((particles << 10) | (1023u - label)) : SBQ_NONE; }
SB_DEV uint32_t sbq_rank_label(uint32_t rkey) { return 1023u - (~rkey & 1023u); }
