"""numpy restatement of hydra's sparse genotype files, written from the format's table, not from the library.

For N individuals and M markers, per class c in ("1", "2", "m") (genotype 1, genotype 2, missing call):
  sl<c>  M uint64   entries of the marker
  ss<c>  M uint64   absolute position of the marker's first entry in si<c> (the exclusive prefix sum of sl<c>)
  si<c>  uint32     0-based row indices, ascending within a marker, markers in .bim order
and .dim is the text "N M\\n".  A row's 2-bit field of the BED byte (row i: byte i // 4, bits 2 * (i % 4)) holds the A1 count:
0b00 -> 2, 0b10 -> 1, 0b11 -> 0, 0b01 -> missing.  Genotype 0 is stored nowhere.
"""
import numpy as np

CLASSES = ("1", "2", "m")
_FIELD_OF_CLASS = {"1": 0b10, "2": 0b00, "m": 0b01}


def _fields(bed, N):
    bed = np.asarray(bed, dtype=np.uint8)
    M = bed.shape[0]
    return np.stack([(bed >> (2 * s)) & 3 for s in range(4)], axis=2).reshape(M, -1)[:, :N]


def bed_to_lists(bed, N):
    """(M, ceil(N/4)) BED columns -> {"sl1", "ss1", "si1", "sl2", ...}"""
    f = _fields(bed, N)
    out = {}
    for c in CLASSES:
        hit = f == _FIELD_OF_CLASS[c]
        sl = hit.sum(axis=1).astype(np.uint64)
        ss = np.zeros_like(sl)
        if sl.size:
            ss[1:] = np.cumsum(sl)[:-1]
        # (np.nonzero walks row-major: markers in order, rows ascending within a marker)
        out["sl" + c], out["ss" + c], out["si" + c] = sl, ss, np.nonzero(hit)[1].astype(np.uint32)
    return out


def lists_to_bed(lists, N, M):
    """the inverse: (M, ceil(N/4)) BED columns; the slots of the last byte beyond N hold the missing code"""
    nb = (N + 3) // 4
    f = np.full((M, nb * 4), 0b11, dtype=np.uint8)
    f[:, N:] = 0b01
    for c in CLASSES:
        ss, sl, si = lists["ss" + c], lists["sl" + c], lists["si" + c]
        for j in range(M):
            rows = si[int(ss[j]):int(ss[j]) + int(sl[j])]
            assert np.all(f[j, rows] == 0b11), "marker %d: a row is listed twice" % j
            f[j, rows] = _FIELD_OF_CLASS[c]
    f = f.reshape(M, nb, 4)
    return np.ascontiguousarray(f[:, :, 0] | (f[:, :, 1] << 2) | (f[:, :, 2] << 4) | (f[:, :, 3] << 6), dtype=np.uint8)


def file_bytes(lists, N, M):
    """suffix -> content of the ten files"""
    out = {"dim": ("%d %d\n" % (N, M)).encode()}
    for c in CLASSES:
        out["sl" + c] = np.asarray(lists["sl" + c], dtype=np.uint64).tobytes()
        out["ss" + c] = np.asarray(lists["ss" + c], dtype=np.uint64).tobytes()
        out["si" + c] = np.asarray(lists["si" + c], dtype=np.uint32).tobytes()
    return out


def write_files(prefix, lists, N, M):
    for suffix, content in file_bytes(lists, N, M).items():
        with open(prefix + "." + suffix, "wb") as f:
            f.write(content)
