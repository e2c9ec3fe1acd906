"""What the device sort (csrc/fx_sort_kernel.h) must answer, in plain NumPy, the sizes at which it changes its
code path, and the cost planes written for it beside the 14 of tests/device_planes.py.  Importable without a GPU.

The rule: the pool is (flags & require) == require and (flags & exclude) == 0; its order is pool[np.argsort(cost[pool],
kind="stable")] -- cost ascending, ties by index, -0.0 == +0.0, every NaN behind +inf in index order."""
import os
import re

import numpy as np

from frenetix_motion_planner_amd import _abi, synthetic
from tests import device_planes as dp

CSRC = os.path.join(os.path.dirname(os.path.abspath(synthetic.__file__)), "csrc")
COSTED, SEL, COL, BND = _abi.FX_FLAG_COSTED, _abi.FX_FLAG_SELECTABLE, _abi.FX_FLAG_COLLISION, _abi.FX_FLAG_BOUNDARY

# ---- the sizes at which the kernels change their code path (tests/test_sort_host.py::test_switch_sizes_follow_the_source derives
# each of them from the #defines of csrc/fx_sort_kernel.h and fails when one moves) ----
SORT_SMALL_MAX = 4_096      # largest agent one workgroup sorts in LDS in one launch
SORT_TILE = 2_048           # keys per tile of the general decomposition (256 lanes x 8 keys)
SORT_DIGIT_BITS = 8
SORT_WAVE_RUN = 512         # consecutive keys of a tile that one wave ranks (8 rounds of 64)
SORT_SIZES = (1, 63, 64, 65,                                            # one wave's lanes
              SORT_TILE - 1, SORT_TILE, SORT_TILE + 1,                  # one tile (the one-workgroup kernel: a round more at + 1)
              SORT_SMALL_MAX, SORT_SMALL_MAX + 1,                       # the last one-workgroup agent; three tiles, the last of ONE key
              3 * SORT_TILE - 1, 3 * SORT_TILE, 3 * SORT_TILE + 1,      # whole tiles of the general decomposition and one key more
              199_999)                                                  # 98 tiles, the last ragged (as in device_planes.TOPK_SIZES)
POOLS = ((COSTED, 0), (SEL, COL | BND), (0, 0))                         # sorted_ids(); the top-k's survivors; every candidate

KEY_NAN = np.uint64(0xFFF0000000000001)
KEY_OUT = np.uint64(0xFFFFFFFFFFFFFFFF)


def source_constants() -> dict:
    """the #defines of csrc/fx_sort_kernel.h the sizes above follow from, and the two places that must agree with them"""
    hdr = open(os.path.join(CSRC, "fx_sort_kernel.h")).read()
    kern = open(os.path.join(CSRC, "fx_kernels.hip")).read()
    api = open(os.path.join(CSRC, "fx_api_sort.hip")).read()

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]

    out = {name.lower(): int(one(rf"#define FX_SORT_{name} (\d+)\b", hdr)) for name in ("BLOCK", "DIGIT_BITS", "ITEMS", "TILE", "SMALL_MAX")}
    out["key_nan"] = int(one(r"#define FX_SORT_KEY_NAN (0x[0-9A-F]+)ULL", hdr), 16)
    out["key_out"] = int(one(r"#define FX_SORT_KEY_OUT (0x[0-9A-F]+)ULL", hdr), 16)
    # the host half sizes its buffers by the same #define: it includes the header without the kernels
    assert "#define FX_SORT_DEFINES_ONLY" in api and '#include "fx_sort_kernel.h"' in api and "/ FX_SORT_TILE);" in api
    assert not re.search(r"\b2048\b", api)
    assert one(r"if \(max_C (<=?) FX_SORT_SMALL_MAX\)", kern) == "<="          # the launcher's switch, as written
    assert "static_assert(FX_SORT_TILE == FX_SORT_BLOCK * FX_SORT_ITEMS" in hdr
    return out


# ---- the references ----
def pool_mask(flags, require, exclude):
    return ((flags & np.uint32(require)) == np.uint32(require)) & ((flags & np.uint32(exclude)) == 0)


def reference_order(cost, flags, require, exclude):
    """(ids by rank, n_nan): THE reference of the GPU module"""
    pool = np.nonzero(pool_mask(flags, require, exclude))[0]
    return pool[np.argsort(cost[pool], kind="stable")], int(np.isnan(cost[pool]).sum())


def sort_keys(cost, flags, require, exclude):
    """NumPy restatement of fx_sort_key: the 64-bit key of every candidate"""
    b = dp.bits(cost).copy()
    nan = (b & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)
    b[b == np.uint64(0x8000000000000000)] = np.uint64(0)
    k = np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(0x8000000000000000))
    k[nan] = KEY_NAN
    k[~pool_mask(flags, require, exclude)] = KEY_OUT
    return k


def radix_order(keys):
    """what eight stable passes over the 8-bit digits of the keys, least significant first, leave: the candidate at every rank"""
    order = np.arange(len(keys))
    for p in range(64 // SORT_DIGIT_BITS):
        digit = (keys[order] >> np.uint64(p * SORT_DIGIT_BITS)) & np.uint64((1 << SORT_DIGIT_BITS) - 1)
        order = order[np.argsort(digit, kind="stable")]
    return order


# ---- planes written for the sort (each a function of the candidate count; seeded) ----
_MIXED_FLAGS = np.array([COSTED | SEL, COSTED, SEL | COL | COSTED, SEL, 0, SEL | BND | COSTED, _abi.FX_FLAG_VALID | COSTED | SEL], np.uint32)
BYTE_BASE = 0x4010203040506070      # a positive finite double; "byte_k" planes vary byte k of it


def extra_plane(name: str, n: int):
    """(cost, flags): flags mix every pool of POOLS into a proper subset; the costs are what the name says"""
    rng = np.random.default_rng([20251019, n, sum(name.encode())])
    flags = rng.choice(_MIXED_FLAGS, size=n)
    ids = np.arange(n)
    if name.startswith("byte_"):                   # keys that differ in exactly ONE byte: a skipped or misordered pass shows
        k = int(name[5:])
        digit = rng.integers(0, 128 if k == 7 else 256, size=n, dtype=np.uint64)     # (byte 7: the sign stays clear, the exponent finite)
        b = (np.uint64(BYTE_BASE) & ~(np.uint64(0xFF) << np.uint64(8 * k))) | (digit << np.uint64(8 * k))
        cost = b.view(np.float64)
    elif name == "digits_0_255":                   # digit values 0 and 255 in every byte of the key
        b = np.zeros(n, np.uint64)
        for k in range(7):
            b |= rng.choice(np.array([0x00, 0xFF], np.uint64), size=n) << np.uint64(8 * k)
        b |= rng.choice(np.array([0x00, 0x7F, 0x80, 0xFF], np.uint64), size=n) << np.uint64(56)   # key bytes 0x80, 0xFF, 0x7F, 0x00
        cost = b.view(np.float64)
    elif name == "one_bucket_but_one":             # every pass: one bucket holds everything (larger than a tile) except one candidate
        cost = np.full(n, 1.5)
        cost[n // 2] = -7.25
        flags[n // 2] = COSTED | SEL
    elif name == "descending":                     # strictly descending through zero: every candidate moves
        cost = (n // 2 - ids).astype(np.float64) * 0.25 + 0.125
    elif name == "signs_interleaved":              # negative and positive interleaved, +-0 as neighbours, subnormals
        cyc = np.array([-1.5, 2.0, -0.0, 0.0, 5e-324, -5e-324, 0.0, -0.0, 1e-310, -1e-310, -2.0, 1.5, np.inf, -np.inf])
        cost = cyc[ids % len(cyc)].copy()
        at = rng.uniform(size=n) < 0.3
        cost[at] = rng.normal(size=int(at.sum())) * 1e-3
    elif name == "nan_between":                    # pool NaNs of both signs, with payloads, between finite costs
        cost = rng.normal(size=n)
        at = rng.uniform(size=n) < 0.3
        cost[at] = dp._nan_payloads(rng, int(at.sum()))
        if n > 2:
            cost[1], flags[1] = dp._nan_payloads(rng, 1)[0], COSTED | SEL       # (a NaN in front of finite costs, in every pool)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(cost, dtype=np.float64), np.ascontiguousarray(flags, dtype=np.uint32)


EXTRA_PLANES = tuple(f"byte_{k}" for k in range(8)) + ("digits_0_255", "one_bucket_but_one", "descending", "signs_interleaved",
                                                         "nan_between")


def any_plane(name: str, n: int):
    return dp.plane(name, n) if name in dp.PLANES else extra_plane(name, n)


ALL_PLANES = dp.PLANES + EXTRA_PLANES
