"""Numpy model of the training-state file (TEST INFRASTRUCTURE): the segment layout, the digest, the packed payload and
the file around it.  Written from the format's description, not from the product code.

File: bytes 0..7 the magic NSFSTATE, u32 format version (1), u32 header length, the UTF-8 JSON header (sorted keys),
zero padding up to a multiple of 256, then the payload.  Payload: segment k starts at align256(end of the stored
segment before it); padding bytes are zero.  Digest of a segment, its bytes read as little-endian 32-bit words
w_0 .. w_{n-1}:  A = sum w_i mod 2^64,  B = sum (i + 1) w_i mod 2^64."""
import json
import struct

import numpy as np

MAGIC = b"NSFSTATE"
VERSION = 1
KNOWN_ANSWER = (8648654848, 39057358848)        # of the bytes of float32 [1..8]


def align256(n):
    return (int(n) + 255) // 256 * 256


def layout(sizes):
    """(offsets, total bytes) of segments of the given sizes (every size a multiple of 4)."""
    offs, end = [], 0
    for b in sizes:
        if b < 0 or b % 4:
            raise ValueError("segment size %r is not a multiple of 4" % (b,))
        end = align256(end)
        offs.append(end)
        end += int(b)
    return offs, end


def digest(buf):
    """(A, B) of a bytes-like object or array (its bytes).  numpy uint64 wraps silently: that is the arithmetic."""
    raw = np.frombuffer(np.ascontiguousarray(buf).tobytes() if isinstance(buf, np.ndarray) else bytes(buf), dtype=np.uint8)
    if raw.size % 4:
        raise ValueError("segment size %d is not a multiple of 4" % raw.size)
    w = raw.view("<u4").astype(np.uint64)
    with np.errstate(over="ignore"):
        i1 = np.arange(1, w.size + 1, dtype=np.uint64)
        return int(w.sum(dtype=np.uint64)), int((i1 * w).sum(dtype=np.uint64))


def pack(arrays, stored=None):
    """(payload bytes, offsets, digests) of the arrays; stored[k] False: digest only (offset -1, no bytes)."""
    stored = [True] * len(arrays) if stored is None else list(stored)
    raws = [np.ascontiguousarray(a).tobytes() for a in arrays]
    offs, total = layout([len(r) if s else 0 for r, s in zip(raws, stored)])
    out = bytearray(total)
    for r, s, o in zip(raws, stored, offs):
        if s:
            out[o:o + len(r)] = r
    return bytes(out), [o if s else -1 for o, s in zip(offs, stored)], [digest(r) for r in raws]


def file_bytes(header, payload):
    """The file of a header dict and a payload."""
    h = json.dumps(header, sort_keys=True, separators=(",", ":")).encode("utf-8")
    head = MAGIC + struct.pack("<II", VERSION, len(h)) + h
    return head + b"\0" * (align256(len(head)) - len(head)) + payload


def parse(raw):
    """(header dict, payload bytes) of a file's bytes."""
    if raw[:8] != MAGIC:
        raise ValueError("bad magic")
    version, n = struct.unpack("<II", raw[8:16])
    if version != VERSION:
        raise ValueError("bad version %d" % version)
    return json.loads(raw[16:16 + n].decode("utf-8")), raw[align256(16 + n):]
