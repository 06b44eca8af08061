"""TEST INFRASTRUCTURE: golden fixtures stored as several .npz parts of at most 1 MiB each.

`save(path, arrays)` writes `<stem>.partNN.npz` next to where `path` (`<stem>.npz`) would be: arrays are packed into
parts by compressed size, and an array too large for one part is cut along one axis into pieces stored under
`<key>::<axis>::<index>`.  `load(path)` reads `path` itself when it exists, else its parts, and gives back a read-only
mapping with the `.files` / `[key]` / `in` interface of `np.load`, every array bit-identical to what was saved."""
import glob
import io
import math
import os
import re
import zipfile

import numpy as np

LIMIT = 1 << 20          # bytes per committed file
_BUDGET = 900 * 1024     # compressed bytes per part (leaves room for the zip directory)
_PIECE = re.compile(r"^(.*)::(\d+)::(\d+)$")


def _parts_of(path):
    stem = path[:-4] if path.endswith(".npz") else path
    return sorted(glob.glob(glob.escape(stem) + ".part[0-9][0-9].npz"))


def _csize(a):
    buf = io.BytesIO()
    np.savez_compressed(buf, a=a)
    return buf.tell()


def _pieces(key, a):
    """(key, array, compressed bytes) pieces of one array, each under the part budget."""
    c = _csize(a)
    if c <= _BUDGET:
        return [(key, a, c)]
    n = math.ceil(c / (0.8 * _BUDGET))
    while True:
        axis = next((i for i, s in enumerate(a.shape) if s >= n), None)
        if axis is None:
            raise ValueError(f"{key}: {a.shape} cannot be cut into {n} pieces along one axis")
        ps = [np.ascontiguousarray(p) for p in np.array_split(a, n, axis=axis)]
        cs = [_csize(p) for p in ps]
        if max(cs) <= _BUDGET:
            return [(f"{key}::{axis}::{i}", p, c) for i, (p, c) in enumerate(zip(ps, cs))]
        n += 1


def save(path, arrays):
    """Write `arrays` (name -> array) as `<stem>.partNN.npz`, removing older parts and `path` itself."""
    for old in _parts_of(path) + ([path] if os.path.exists(path) else []):
        os.remove(old)
    pieces = [p for k, a in arrays.items() for p in _pieces(k, np.asarray(a))]
    bins = []   # first-fit decreasing by compressed size
    for key, a, c in sorted(pieces, key=lambda p: -p[2]):
        for b in bins:
            if b[0] + c <= _BUDGET:
                b[0] += c
                b[1][key] = a
                break
        else:
            bins.append([c, {key: a}])
    stem = path[:-4] if path.endswith(".npz") else path
    written = []
    for i, (_, d) in enumerate(bins):
        name = f"{stem}.part{i:02d}.npz"
        np.savez_compressed(name, **d)
        assert os.path.getsize(name) < LIMIT, (name, os.path.getsize(name))
        written.append(name)
    return written


class Parts:
    """The arrays of one fixture, read from its parts (pieces joined again on first access)."""

    def __init__(self, paths):
        self._where, pieces = {}, {}
        for p in paths:
            with zipfile.ZipFile(p) as z:
                for n in z.namelist():
                    key = n[:-4]
                    m = _PIECE.match(key)
                    if m:
                        pieces.setdefault(m.group(1), []).append((int(m.group(3)), int(m.group(2)), p, key))
                    else:
                        self._where[key] = p
        self._pieces = {k: sorted(v) for k, v in pieces.items()}
        self.files = sorted(set(self._where) | set(self._pieces))
        self._cache = {}

    def _read(self, path, key):
        with np.load(path) as z:
            return z[key]

    def __getitem__(self, key):
        if key not in self._cache:
            if key in self._where:
                self._cache[key] = self._read(self._where[key], key)
            elif key in self._pieces:
                ps = self._pieces[key]
                self._cache[key] = np.concatenate([self._read(p, k) for _, _, p, k in ps], axis=ps[0][1])
            else:
                raise KeyError(key)
        return self._cache[key]

    def __contains__(self, key):
        return key in self._where or key in self._pieces

    def __iter__(self):
        return iter(self.files)

    def keys(self):
        return list(self.files)


def load(path):
    """np.load(path) if that file exists, else the fixture assembled from its parts."""
    if os.path.exists(path):
        return np.load(path)
    paths = _parts_of(path)
    if not paths:
        raise FileNotFoundError(f"{path}: neither the file nor {os.path.basename(path)[:-4]}.partNN.npz parts exist")
    return Parts(paths)
