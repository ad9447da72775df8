"""TEST INFRASTRUCTURE for the block-batch cases of tests/test_simt_packed.py (packed encode) and tests/test_simt_compact.py (compact
decode), which are one design: the mixed lengths of a batch, its rounds, the info record that follows from per-block results, the two
source layouts with the Batch descriptor over them, and the output arrays of a call between sentinel values."""
import numpy as np

from lz4net_amd._lib import Batch

SMALL = (0, 1, 12, 13, 64)


def lengths_of(n):
    """mixed lengths: mostly the short ones, the long ones at the ends and around the round boundaries, ONE block of 70 000"""
    lens = [SMALL[(i * 7 + i // 5) % len(SMALL)] for i in range(n)]
    for i, length in ((0, 65536), (n - 1, 4096), (2, 70000), (63, 4096), (64, 65536), (255, 4096), (256, 4096), (999, 65536), (1000, 4096),
                      (4095, 4096), (4096, 65536)):
        if 0 <= i < n and (length != 70000 or n > 2):
            lens[i] = length
    if n == 1:
        lens[0] = 70000
    return lens


def rounds_of(n, k):
    k = n if k <= 0 or k > n else k
    return (0, 0) if n == 0 else ((n + k - 1) // k, k)


def expect_info(n, res, offs, dst_cap, failed):
    """(blocks, total bytes, written blocks, first failed block, its result); failed(result) says which results count as failures: an
    encoder's 0 (no room) does, a decoder's 0 (an empty block) does not"""
    bad = [i for i in range(n) if failed(res[i])]
    written = max(w for w in range(n + 1) if offs[w] <= dst_cap)
    return (n, int(offs[n]), written, bad[0] if bad else -1, int(res[bad[0]]) if bad else 0)


class BlockCase:
    """n rows in one of the two source layouts, and the Batch descriptor over them"""

    def lay_out(self, rows, src_len, layout, src_len_all, dst_cap_all):
        n = self.n = len(rows)
        self.src_len = np.array(list(src_len) + [0], np.int32)
        self.src_len_all, self.dst_cap_all = src_len_all, dst_cap_all
        longest = max([r.size for r in rows] + [1])
        if layout == "strided":
            self.stride = longest + 7
            self.src = np.full(max(n, 1) * self.stride + 16, 0x77, np.uint8)
            for i, r in enumerate(rows):
                self.src[i * self.stride:i * self.stride + r.size] = r
            self.src_off = None
        else:
            # rows in reverse order with gaps: offsets that do not increase
            self.stride = 0
            self.src_off = np.zeros(n + 1, np.int64)
            at = 3
            for i in reversed(range(n)):
                self.src_off[i] = at
                at += rows[i].size + (i % 5)
            self.src = np.full(at + 16, 0x77, np.uint8)
            for i, r in enumerate(rows):
                self.src[self.src_off[i]:self.src_off[i] + r.size] = r

    def batch(self, caps=None, result=None, uniform_len=None):
        b = Batch()
        b.src, b.src_stride = self.src.ctypes.data, self.stride
        b.src_off = None if self.src_off is None else self.src_off.ctypes.data
        b.src_len = None if uniform_len is not None else self.src_len.ctypes.data
        b.src_len_all = uniform_len if uniform_len is not None else self.src_len_all
        b.dst, b.dst_off, b.dst_stride = None, None, 0
        b.dst_cap = None if caps is None else caps.ctypes.data
        b.dst_cap_all = self.dst_cap_all
        b.result = None if result is None else result.ctypes.data
        b.n_blocks = self.n
        return b


def sentinels(n, info_type):
    """(dst_off, lengths, results, info) of one call: the n + 1 offsets and the n lengths and results start at element 1"""
    return np.full(n + 3, -77, np.int64), np.full(n + 2, -77, np.int32), np.full(n + 2, -77, np.int32), info_type(-7, -7, -7, -7, -7, -7)


def check_sentinels(n, dst_off, lengths, result):
    assert dst_off[0] == -77 and dst_off[n + 2] == -77 and lengths[0] == -77 and lengths[n + 1] == -77 and result[0] == -77 and result[n + 1] == -77
