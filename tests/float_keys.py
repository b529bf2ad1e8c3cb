"""Finite float32 values as uint32 keys of the same order, -0.0 below +0.0 (sbb_fkey of csrc/sb_summary_math.h), and the extremes
taken in that order: what the summary references (batch_summary_ref, batch_body_summary_ref, body_summary_ref) share."""
import numpy as np


def fkey(x):
    b = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def key_min(x):
    return unkey(fkey(x).min())


def key_max(x):
    return unkey(fkey(x).max())
