"""What the reference's OWN code returns, for the tests that compare against it.

Where the reference tree is importable (oracle/ref_import.py) the results are computed live and checked against the
stored copy; everywhere else the stored copy (tests/golden/reference_code/<name>.pkl.gz: builtins and numpy only,
`TextBlock`s as namespaces of their detection fields) stands in for them, so these tests run on every machine.
`CTD_RECORD_REFERENCE=1 python -m pytest tests/...` (re)writes the stored copies from the live reference."""
import gzip
import hashlib
import io
import os
import pickle
import types

import numpy as np
import torch

from conftest import GOLDEN
from oracle import ref_import as RI

DIR = os.path.join(GOLDEN, "reference_code")
BLOCK_FIELDS = ("xyxy", "lines", "language", "vertical", "angle", "merged", "font_size", "distance", "vec", "norm", "weight")
_POST = []


def reference_post():
    """The reference's post-processing modules (oracle/ref_post_import.py); only where the tree is present."""
    if not _POST:
        from oracle import ref_post_import as RP
        _POST.append(RP.load_reference_post())
    return _POST[0]


def sha256(a) -> str:
    a = np.ascontiguousarray(a)
    return f"{a.dtype.str}{a.shape}:" + hashlib.sha256(a.tobytes()).hexdigest()


def plain(x):
    """Tensors -> numpy, TextBlocks -> namespaces of BLOCK_FIELDS, containers recursively; scalars keep their type."""
    if isinstance(x, torch.Tensor):
        return x.detach().numpy().copy()
    if isinstance(x, np.ndarray):
        return x.copy()
    if isinstance(x, (list, tuple)):
        return type(x)(plain(v) for v in x)
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if hasattr(x, "xyxy") and hasattr(x, "lines") and hasattr(x, "font_size"):
        return types.SimpleNamespace(**{k: plain(getattr(x, k)) for k in BLOCK_FIELDS})
    return x


def same(a, b) -> bool:
    """Exact equality of two `plain` values: types, shapes, dtypes and every bit (NaN equals NaN)."""
    if type(a) is not type(b):
        return False
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, types.SimpleNamespace):
        return same(vars(a), vars(b))
    if isinstance(a, (float, np.floating)) and a != a:
        return b != b
    return bool(a == b)


def _load(path):
    with gzip.open(path, "rb") as f:
        return pickle.load(f)


def _store(path, value) -> None:
    buf = io.BytesIO()
    with gzip.GzipFile(fileobj=buf, mode="wb", mtime=0) as f:            # the same bytes for the same results
        pickle.dump(value, f, protocol=4)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(buf.getvalue())


def reference_results(name: str, compute):
    """`plain(compute())` -- `compute` calls the reference's code -- live where the reference is present, else stored."""
    path = os.path.join(DIR, name + ".pkl.gz")
    if not RI.reference_available():
        return _load(path)
    live = plain(compute())
    if os.environ.get("CTD_RECORD_REFERENCE"):
        _store(path, live)
    else:
        assert same(_load(path), live), f"{path} no longer holds what the reference's code returns (CTD_RECORD_REFERENCE=1)"
    return live
