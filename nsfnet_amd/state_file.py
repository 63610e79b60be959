"""The training-state file: one file per rank.

  bytes 0..7   the magic NSFSTATE
  u32          format version (1)
  u32          header length
  header       UTF-8 JSON, sorted keys, nothing that depends on the time or the host
  padding      zeros up to a multiple of 256
  payload      the packed buffer: segment k at align256(end of the stored segment before it), zero padding

Two snapshots of one state are byte-identical files.  Header keys: segments (name, dtype, shape, bytes, offset - -1 for
a segment that is digested but not stored -, digest [A, B]), fingerprint (structural: a difference refuses the load),
info (recorded: differences are reported), host (the host mirrors) and extra (the caller's dict)."""
import ctypes
import json
import os
import struct

import numpy as np

from . import _lib

MAGIC = b"NSFSTATE"
VERSION = 1


class StateFileError(RuntimeError):
    """The file is not a whole, undamaged training-state file."""


def align256(n):
    return (int(n) + 255) // 256 * 256


def layout(sizes):
    """pinn_state_layout: (offsets, total bytes) of segments of the given sizes."""
    n = len(sizes)
    b = (ctypes.c_int64 * max(n, 1))(*[int(s) for s in sizes])
    o = (ctypes.c_int64 * max(n, 1))()
    total = int(_lib.load().pinn_state_layout(n, b, o))
    if total < 0:
        raise ValueError("training state: %s" % _lib.load().pinn_last_error().decode())
    return [int(v) for v in o[:n]], total


def digest_host(buf):
    """pinn_state_digest_host: (A, B) of a contiguous uint8 numpy array."""
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    out = (ctypes.c_uint64 * 2)()
    _lib.check(_lib.load().pinn_state_digest_host(ctypes.c_void_p(buf.ctypes.data if buf.size else 0), buf.size, out),
               "pinn_state_digest_host")
    return int(out[0]), int(out[1])


def encode_header(header):
    h = json.dumps(header, sort_keys=True, separators=(",", ":")).encode("utf-8")
    head = MAGIC + struct.pack("<II", VERSION, len(h)) + h
    return head + b"\0" * (align256(len(head)) - len(head))


def write(path, header, payload):
    """Write path + '.tmp', then os.replace: a writer that dies leaves the previous file whole."""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(encode_header(header))
        f.write(memoryview(payload))
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def read_header(path):
    """The header alone, unverified beyond the magic and the version."""
    with open(path, "rb") as f:
        head = f.read(16)
        if len(head) < 16 or head[:8] != MAGIC or struct.unpack("<II", head[8:])[0] != VERSION:
            raise StateFileError("%s: not a training-state file of format version %d" % (path, VERSION))
        try:
            return json.loads(f.read(struct.unpack("<II", head[8:])[1]).decode("utf-8"))
        except ValueError as e:
            raise StateFileError("%s: unreadable header (%s)" % (path, e))


def read(path):
    """(header, payload as a uint8 numpy array) of a verified file: the magic, the version, the length of the payload
    and the digest of every stored segment are checked here, on the host.  StateFileError otherwise."""
    with open(path, "rb") as f:
        head = f.read(16)
        if len(head) < 16 or head[:8] != MAGIC:
            raise StateFileError("%s: not a training-state file (bad magic)" % path)
        version, n = struct.unpack("<II", head[8:])
        if version != VERSION:
            raise StateFileError("%s: format version %d (this build reads %d)" % (path, version, VERSION))
        raw = f.read(n)
        if len(raw) < n:
            raise StateFileError("%s: truncated inside the header" % path)
        try:
            header = json.loads(raw.decode("utf-8"))
            segs = header["segments"]
            stored = [s for s in segs if s["offset"] >= 0]
            offs, total = layout([s["bytes"] if s["offset"] >= 0 else 0 for s in segs])
            if [s["offset"] for s in segs] != [o if s["offset"] >= 0 else -1 for o, s in zip(offs, segs)]:
                raise ValueError("the segment offsets are not the layout of their sizes")
        except (ValueError, KeyError, TypeError) as e:
            raise StateFileError("%s: unreadable header (%s)" % (path, e))
        f.seek(align256(16 + n))
        payload = np.fromfile(f, dtype=np.uint8)
    if payload.size != total:
        raise StateFileError("%s: the payload has %d bytes, the header describes %d (truncated?)"
                             % (path, payload.size, total))
    for s in stored:
        d = digest_host(payload[s["offset"]:s["offset"] + s["bytes"]])
        if list(d) != [int(v) for v in s["digest"]]:
            raise StateFileError("%s: segment %r does not match its digest (file %s, header %s)"
                                 % (path, s["name"], list(d), s["digest"]))
    return header, payload
