"""CPU-only: what the Python front end (lz4net_amd/{stream,wrap,legacy_frame,lz4_frame}.py) refuses before it reaches the library, and
the exceptions it maps the library's status codes to -- type, text and attributes.  No kernel runs: every call here must raise in the
front's own checks, which is why tensors that only CLAIM to be on a GPU are enough."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lz4net_amd import _lib, legacy_frame as lf, lz4_frame as lz, stream as st, wrap
from lz4net_amd.codec import ArgumentException
from lz4net_amd.stream import EndOfStreamException

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _OnGpu0(torch.Tensor):
    """a CPU tensor that answers .is_cuda and .device as one on cuda:0 would"""
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", 0))


class _OnGpu1(torch.Tensor):
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", 1))


def gpu(t, cls=_OnGpu0):
    return t.as_subclass(cls)


def u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8)


def i64(*values):
    return torch.tensor(values, dtype=torch.int64)


BYTES, OFFS, OUT = gpu(u8(64)), gpu(i64(0, 32, 64)), gpu(u8(256))
BEGIN, END = gpu(i64(0, 32)), gpu(i64(32, 64))


def refused(text, fn, *args, **kwargs):
    with pytest.raises(ArgumentException) as e:
        fn(*args, **kwargs)
    assert type(e.value) is ArgumentException and str(e.value) == text, (fn.__name__, str(e.value))
    return e.value


def test_the_stand_in_tensors_pass_the_checks_real_ones_would():
    assert BYTES.is_cuda and BYTES.contiguous().is_cuda and BYTES.device == OUT.device != gpu(u8(4), _OnGpu1).device
    assert not u8(4).is_cuda


# ---- one buffer of device bytes ----------------------------------------------------------------------------------------------------
BYTES_FRONTS = [
    ("t", st.compress_stream_device), ("t", st.decompress_stream_device), ("t", st.stream_directory),
    ("t", lambda t: st.decompress_stream_into(t, OUT)), ("t", lambda t: st.decompress_stream_range(t, None, 0, 0)),
    ("t", lf.compress_frame_device), ("t", lf.decompress_frame_device), ("t", lf.decompress_frame_compact_device),
    ("t", lz.compress_frame_device), ("t", lz.decompress_frame_device),
    ("data", lambda t: lz.xxh32_rows_device(t, gpu(i64(0)), gpu(torch.zeros(1, dtype=torch.int32)))),
]
NOT_DEVICE_BYTES = {"a CPU tensor": u8(64), "the wrong dtype": gpu(torch.zeros(64, dtype=torch.int32)), "two dimensions": gpu(u8(8, 8)),
                    "no tensor": np.zeros(64, np.uint8)}


@pytest.mark.parametrize("bad", list(NOT_DEVICE_BYTES))
@pytest.mark.parametrize("front", range(len(BYTES_FRONTS)))
def test_device_bytes(front, bad):
    name, fn = BYTES_FRONTS[front]
    refused(f"{name} must be a 1-D uint8 CUDA tensor", fn, NOT_DEVICE_BYTES[bad])


# ---- batches: a buffer and offsets[n + 1] ----------------------------------------------------------------------------------------
BATCH_FRONTS = [st.compress_streams_device, st.decompress_streams_device, lambda b, o: st.decompress_streams_into(b, o, OUT),
                wrap.wrap_device, wrap.unwrap_device, lambda b, o: wrap.unwrap_into(b, o, OUT)]


@pytest.mark.parametrize("front", range(len(BATCH_FRONTS)))
def test_device_batch(front):
    fn = BATCH_FRONTS[front]
    for bad in ("a CPU tensor", "the wrong dtype", "two dimensions", "no tensor"):
        refused("the buffer must be a 1-D uint8 CUDA tensor", fn, NOT_DEVICE_BYTES[bad], OFFS)
    for bad in (i64(0, 64), gpu(torch.zeros(3, dtype=torch.int32)), gpu(i64(0, 64).reshape(1, 2)), np.zeros(3, np.int64)):
        refused("offsets must be a 1-D int64 CUDA tensor", fn, BYTES, bad)
    refused("offsets must hold n + 1 entries", fn, BYTES, gpu(i64()))
    refused("the buffer and the offsets must be on the same device", fn, BYTES, gpu(i64(0, 64), _OnGpu1))


# ---- chosen items: a buffer, begin[m] and end[m] ---------------------------------------------------------------------------------
SPANS_FRONTS = [lambda b, s, e: st.decompress_streams_spans_into(b, s, e, OUT), lambda b, s, e: wrap.unwrap_spans_into(b, s, e, OUT)]


@pytest.mark.parametrize("front", range(len(SPANS_FRONTS)))
def test_device_spans(front):
    fn = SPANS_FRONTS[front]
    for bad in ("a CPU tensor", "the wrong dtype", "two dimensions", "no tensor"):
        refused("the buffer must be a 1-D uint8 CUDA tensor", fn, NOT_DEVICE_BYTES[bad], BEGIN, END)
    for bad in (i64(0, 32), gpu(torch.zeros(2, dtype=torch.int32)), gpu(i64(0, 32).reshape(1, 2)), np.zeros(2, np.int64)):
        refused("begin and end must be 1-D int64 CUDA tensors", fn, BYTES, bad, END)
        refused("begin and end must be 1-D int64 CUDA tensors", fn, BYTES, BEGIN, bad)
    refused("the buffer and the spans must be on the same device", fn, BYTES, gpu(i64(0, 32), _OnGpu1), END)
    refused("the buffer and the spans must be on the same device", fn, BYTES, BEGIN, gpu(i64(32, 64), _OnGpu1))
    refused("begin and end must have the same length", fn, BYTES, BEGIN, gpu(i64(32)))


# ---- the caller's output tensor ------------------------------------------------------------------------------------------------------
OUT_FRONTS = [lambda out: st.decompress_stream_into(BYTES, out), lambda out: st.decompress_streams_into(BYTES, OFFS, out),
              lambda out: st.decompress_streams_spans_into(BYTES, BEGIN, END, out), lambda out: wrap.unwrap_into(BYTES, OFFS, out),
              lambda out: wrap.unwrap_spans_into(BYTES, BEGIN, END, out)]


@pytest.mark.parametrize("front", range(len(OUT_FRONTS)))
def test_out(front):
    fn = OUT_FRONTS[front]
    for bad in (u8(256), gpu(torch.zeros(256, dtype=torch.int32)), gpu(u8(16, 16)), gpu(u8(512)[::2]), np.zeros(256, np.uint8)):
        refused("out must be a contiguous 1-D uint8 CUDA tensor", fn, bad)
    refused("out must be on the source's device", fn, gpu(u8(256), _OnGpu1))


# ---- the fronts that check by hand -------------------------------------------------------------------------------------------------
def test_select_spans():
    sel = gpu(i64(1, 0))
    for bad in (i64(0, 32, 64), gpu(torch.zeros(3, dtype=torch.int32)), gpu(i64(0, 64).reshape(1, 2)), np.zeros(3, np.int64)):
        refused("offsets must be a 1-D int64 CUDA tensor", wrap.select_spans, bad, sel)
        refused("sel must be a 1-D int64 CUDA tensor", wrap.select_spans, OFFS, bad)
    refused("offsets must hold n + 1 entries", wrap.select_spans, gpu(i64()), sel)
    refused("offsets and sel must be on the same device", wrap.select_spans, OFFS, gpu(i64(1, 0), _OnGpu1))


def test_xxh32_rows():
    text = "off must be an int64 and lens an int32 CUDA tensor of the same length"
    off, lens = gpu(i64(0, 32)), gpu(torch.zeros(2, dtype=torch.int32))
    refused(text, lz.xxh32_rows_device, BYTES, gpu(torch.zeros(2, dtype=torch.int32)), lens)
    refused(text, lz.xxh32_rows_device, BYTES, off, gpu(i64(32, 32)))
    refused(text, lz.xxh32_rows_device, BYTES, off, gpu(torch.zeros(3, dtype=torch.int32)))
    refused(text, lz.xxh32_rows_device, BYTES, i64(0, 32), lens)
    refused(text, lz.xxh32_rows_device, BYTES, off, torch.zeros(2, dtype=torch.int32))


def test_stream_range_outside_the_stream():
    directory = (None, None, np.array([0, 4, 10], np.int64))
    for start, length in ((-1, 2), (0, -1), (5, 6), (11, 0)):
        refused("the range is outside the stream's 10 decoded bytes", st.decompress_stream_range, BYTES, directory, start, length)


# ---- sizes the formats do not have -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_size", [0, -1, 0x7E000001])
def test_legacy_frame_chunk_size(chunk_size):
    text = "chunk_size must be 1 .. 0x7E000000"
    for fn in (lf.compress_frame_device, lf.decompress_frame_device, lf.decompress_frame_compact_device):
        refused(text, fn, BYTES, chunk_size=chunk_size)
        refused("t must be a 1-D uint8 CUDA tensor", fn, u8(64), chunk_size=chunk_size)          # (the tensor is looked at first)
    for fn in (lf.compress_frame_host, lf.decompress_frame_host):
        refused(text, fn, b"abcd", chunk_size=chunk_size)
        refused(text, fn, np.zeros(4, np.uint8), chunk_size=chunk_size)


@pytest.mark.parametrize("block_size", [0, 65535, 131072, 8388608])
def test_lz4_frame_block_size(block_size):
    text = "block_size must be 65536, 262144, 1048576 or 4194304"
    refused(text, lz.compress_frame_device, BYTES, block_size=block_size)
    refused("t must be a 1-D uint8 CUDA tensor", lz.compress_frame_device, u8(64), block_size=block_size)
    refused(text, lz.compress_frame_host, b"abcd", block_size=block_size)


def test_lz4_frame_of_no_bytes():
    e = refused("not an LZ4 frame: unknown magic number", lz.decompress_frame_host, b"")
    assert (e.error_offset, e.status) == (0, _lib.LZ4F_BAD_MAGIC)


# ---- batches in host memory ----------------------------------------------------------------------------------------------------------
HOST_FRONTS = [st.compress_streams_host, st.decompress_streams_host, wrap.wrap_host, wrap.unwrap_host]


@pytest.mark.parametrize("front", range(len(HOST_FRONTS)))
def test_host_batch(front):
    fn = HOST_FRONTS[front]
    offs = np.array([0, 2, 4], np.int64)
    for bad in (np.zeros(4, np.int8), np.zeros((2, 2), np.uint8), [0, 0, 0, 0], torch.zeros(4, dtype=torch.uint8)):
        refused("the buffer must be a 1-D uint8 array", fn, bad, offs)
    for bad in (np.array([0, 2, 4], np.int32), offs.reshape(1, 3), [0, 2, 4], torch.tensor([0, 2, 4])):
        for buf in (b"abcd", bytearray(b"abcd"), memoryview(b"abcd"), np.zeros(4, np.uint8)):
            refused("offsets must be a 1-D int64 array", fn, buf, bad)
    refused("offsets must hold n + 1 entries", fn, b"abcd", np.zeros(0, np.int64))


@pytest.mark.parametrize("offsets", [[0, 3, 2], [0, 3, 2, 4], [-1, 2, 4], [0, 2, 5], [4, 0]])
def test_host_offsets_that_do_not_fit_the_buffer(offsets):
    refused("offsets are invalid for the given buffer", st.compress_streams_host, b"abcd", np.array(offsets, np.int64))


# ---- status codes -> exceptions ------------------------------------------------------------------------------------------------------
_CORRUPT_BLOCK = "LZ4 block is corrupted, or invalid length has been given."
STREAM_ERRORS = {_lib.STREAM_END_OF_STREAM: (EndOfStreamException, "truncated or corrupted stream"),
                 _lib.STREAM_PASSES: (NotImplementedError, "Chunks with multiple passes are not supported."),
                 _lib.STREAM_CORRUPT_BLOCK: (ArgumentException, _CORRUPT_BLOCK)}


def is_exactly(e, cls, text):
    assert type(e) is cls and str(e) == text, (type(e), str(e))


@pytest.mark.parametrize("status", [-1, 0, 1, 2, 3, 4, 5, 99])
def test_stream_error(status):
    cls, text = STREAM_ERRORS.get(status, (_lib.Lz4HipError, f"stream decode: unexpected outcome {status}"))
    e = st._stream_error(_lib.StreamInfo(error=status, error_offset=1 << 40))
    is_exactly(e, cls, text)
    assert e.error_offset == 1 << 40 and not hasattr(e, "item_index")
    e = st.streams_error(status, 7, 123)
    is_exactly(e, cls, text)
    assert (e.item_index, e.error_offset) == (7, 123)
    assert st.streams_error(np.int32(status), np.int64(7)).error_offset == -1


def test_streams_error_for_bad_offsets():
    e = st.streams_error(_lib.E_ARGUMENT, 3, 55)
    is_exactly(e, ArgumentException, "offsets are invalid for the given buffer")
    assert (e.item_index, e.error_offset) == (3, -1)


UNWRAP_ERRORS = {_lib.WRAP_SIZE_INVALID: "inputBuffer size is invalid",
                 _lib.WRAP_CORRUPT_HEADER: "inputBuffer size is invalid or has been corrupted",
                 _lib.WRAP_CORRUPT_BLOCK: _CORRUPT_BLOCK,
                 _lib.E_ARGUMENT: "offsets are invalid for the given buffer"}


@pytest.mark.parametrize("status", [-1, 0, 1, 2, 3, 4, 99, _lib.E_ARGUMENT, _lib.E_DEVICE])
def test_unwrap_error(status):
    e = wrap.unwrap_error(np.int32(status), np.int64(5))
    is_exactly(e, ArgumentException, UNWRAP_ERRORS.get(status, f"unwrap: unexpected status {status}"))
    assert e.message_index == 5 and not hasattr(e, "error_offset")


LEGACY_ERRORS = {_lib.FRAME_BAD_MAGIC: "Unrecognized header : file cannot be decoded",
                 _lib.FRAME_BAD_SIZE: "chunk size exceeds what a chunk can compress to",
                 _lib.FRAME_CORRUPT_BLOCK: "Decoding Failed ! Corrupted input !"}


@pytest.mark.parametrize("status", [-1, 0, 1, 3, 4, 5, 6, 99])
def test_legacy_frame_error(status):
    e = lf._frame_error(status, 40, 100)
    if status in LEGACY_ERRORS:
        is_exactly(e, ArgumentException, LEGACY_ERRORS[status])
    else:
        is_exactly(e, _lib.Lz4HipError, f"frame decode: unexpected outcome {status}")
    assert e.error_offset == 40 and lf._frame_error(status).error_offset == -1


def test_legacy_frame_error_tells_a_cut_size_field_from_a_cut_payload():
    for error_offset, frame_len, text in ((96, 100, "truncated chunk payload"), (97, 100, "truncated chunk header"),
                                          (99, 100, "truncated chunk header"), (4, 20, "truncated chunk payload")):
        e = lf._frame_error(_lib.FRAME_TRUNCATED, error_offset, frame_len)
        is_exactly(e, ArgumentException, text)
        assert e.error_offset == error_offset
    is_exactly(lf._frame_error(_lib.FRAME_TRUNCATED), ArgumentException, "truncated chunk header")       # (defaults: -1 + 4 > -1)


LZ4F_ERRORS = {
    1: "not an LZ4 frame: unknown magic number",
    2: "frame descriptor: wrong version, reserved bit set or invalid block size",
    3: "frame descriptor: header checksum mismatch",
    4: "frames with linked blocks are not supported: their blocks decode only in order",
    5: "frames with a dictionary ID are not supported",
    6: "the frame's block maximum exceeds the slot it was given",
    7: "truncated frame",
    8: "block size exceeds the frame's block maximum",
    9: "Decoding Failed ! Corrupted input !",
    10: "block checksum mismatch",
    11: "decoded size differs from the frame's content size",
    12: "content checksum mismatch",
}


@pytest.mark.parametrize("status", [-1, 0] + list(range(1, 15)) + [99])
def test_lz4_frame_error(status):
    e = lz._frame_error(np.int32(status), np.int64(77))
    if status in LZ4F_ERRORS:
        is_exactly(e, ArgumentException, LZ4F_ERRORS[status])
    else:
        is_exactly(e, _lib.Lz4HipError, f"lz4 frame decode: unexpected outcome {status}")
    assert (e.error_offset, e.status) == (77, status) and type(e.status) is int
    assert lz._frame_error(status).error_offset == -1


def test_lz4f_codes_are_the_librarys():
    assert [_lib.LZ4F_BAD_MAGIC, _lib.LZ4F_CONTENT_CHECKSUM_ERROR, _lib.LZ4F_TABLE_FULL] == [1, 12, 13]


# ---- the package without torch ---------------------------------------------------------------------------------------------------------
def test_the_front_imports_without_torch():
    code = ("import sys\n"
            "from lz4net_amd import codec, stream, wrap, legacy_frame, lz4_frame\n"
            "assert 'torch' not in sys.modules, 'torch was imported'\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
