"""Inputs and measures shared by test_mine_host.py (CPU) and test_gpu_mine.py (GPU)."""
import numpy as np


def ulp_distance(a, b):
    """distance in float32 ulps (units in the last place, counted over the ordered floats)"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def mining_case(seed, shape):
    rs = np.random.RandomState(seed)
    pred = rs.uniform(0, 1, shape).astype(np.float32)
    ll = (rs.uniform(0, 1, shape) > 0.9).astype(np.uint8)
    ll[rs.uniform(0, 1, shape) > 0.98] = 3           # a label that is neither class
    mm = (rs.uniform(0, 1, shape) > 0.2).astype(np.uint8)
    mm[rs.uniform(0, 1, shape) > 0.97] = 2           # a mask value that is neither 0 nor 1
    return pred, ll, mm
