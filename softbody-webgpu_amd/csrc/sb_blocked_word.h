// sb_blocked_word.h -- the entry word of k_substep_blocked as the kernel holds it in registers, and the LDS planes it addresses.
//
// LDS: four planes of 4-byte words behind ONE byte offset per particle record -- px, py (position, float bits), fx, fy (the
// fixed-point force sums).  A plane is SBW_PLANE dwords, a multiple of 64: record q's four words lie at byte 4 q plus an
// immediate, and two of them are one ds_read2st64_b32 / ds_write2st64_b32 (offsets in units of 64 dwords).  So one register per
// endpoint, 4 A, addresses everything the beam phase touches; before, the positions (8-byte records) wanted 8 A and the sums 4 A.
//
// Words: in HBM, in the plan and everywhere outside the kernel an entry is the WIDE word  A | B << 12 | row << 24  (sb_blocking.h).
// A scene with at most SBW_NARROW_ROWS material rows has the kernel repack its words once per launch into the NARROW word
//   bits 0..13  4 A (bits 0, 1 zero)    bits 14..27  4 B (bits 14, 15 zero)    bits 28..31  row
// whose fields are the byte offsets themselves: one v_and, one v_bfe.  The wide word stays in registers as it is when the scene
// has more rows.  Host and device: tests/blocked_word_check.cpp checks the codec on a CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBW_HD __host__ __device__ __forceinline__
#else
#define SBW_HD inline
#endif

#define SBW_LBITS 12u       // = SB_BK_LBITS (sb_blocked.hip asserts it)
#define SBW_CAP 2690u       // = SB_BK_CAP: LDS records of a workgroup, dummy and padding records included
#define SBW_PLANE 2752u     // dwords per plane: the next multiple of 64 from SBW_CAP
#define SBW_NARROW_ROWS 16u // material rows a narrow word can name
#define SBW_MAT_ROW_BYTES 32u // an LDS material row: 8 floats
enum { SBW_PX = 0, SBW_PY = 1, SBW_FX = 2, SBW_FY = 3 };

static_assert(SBW_PLANE % 64u == 0u && SBW_PLANE >= SBW_CAP && SBW_PLANE - SBW_CAP < 64u, "a plane: the next multiple of 64 dwords");
static_assert(4u * (SBW_CAP - 1u) < (1u << 14), "the last padding record's byte offset fits a narrow field");
static_assert(SBW_CAP - 1u < (1u << SBW_LBITS), "... and its index a wide one");
static_assert(4u * (3u * SBW_PLANE) < (1u << 16), "the furthest plane is inside a DS instruction's 16-bit offset");
static_assert(3u * (SBW_PLANE / 64u) < 256u, "... and inside the 8-bit offsets of the st64 forms");

namespace sbw {

// byte offset of plane `pl` from a record's own byte offset
constexpr uint32_t plane_bytes(uint32_t pl) { return 4u * SBW_PLANE * pl; }

SBW_HD uint32_t pack_wide(uint32_t a, uint32_t b, uint32_t row) { return a | (b << SBW_LBITS) | (row << (2u * SBW_LBITS)); }
SBW_HD uint32_t pack_narrow(uint32_t a, uint32_t b, uint32_t row) { return (a << 2) | (b << 16) | (row << 28); }
// wide -> narrow (row < SBW_NARROW_ROWS, or its high bits are lost): A up by 2, B and the row's low four bits up by 4
SBW_HD uint32_t repack(uint32_t wide) { return ((wide & ((1u << SBW_LBITS) - 1u)) << 2) | ((wide << 4) & 0xFFFF0000u); }

template <bool NARROW> SBW_HD uint32_t held(uint32_t wide) { return NARROW ? repack(wide) : wide; }
// A, B of a wide word: region indices
SBW_HD uint32_t index_a(uint32_t wide) { return wide & ((1u << SBW_LBITS) - 1u); }
SBW_HD uint32_t index_b(uint32_t wide) { return (wide >> SBW_LBITS) & ((1u << SBW_LBITS) - 1u); }
// 4 A, 4 B: a record's byte offset inside a plane;  32 row: a material row's byte offset
template <bool NARROW> SBW_HD uint32_t a4(uint32_t w) { return NARROW ? (w & 0x3FFFu) : (index_a(w) << 2); }
template <bool NARROW> SBW_HD uint32_t b4(uint32_t w) { return NARROW ? ((w >> 14) & 0x3FFFu) : (index_b(w) << 2); }
template <bool NARROW> SBW_HD uint32_t row(uint32_t w) { return NARROW ? (w >> 28) : (w >> (2u * SBW_LBITS)); }
template <bool NARROW> SBW_HD uint32_t row32(uint32_t w) { return row<NARROW>(w) * SBW_MAT_ROW_BYTES; }

} // namespace sbw
