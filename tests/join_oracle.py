"""Brute-force join oracle shared by test_joins.py and
test_gpu_join_family.py: plain Python loops and dicts over the rows, no
searchsorted and nothing from sparkrdma_amd.joins.

Keys are uint64 arrays sorted as unsigned; payloads uint64 arrays or None.
``loop_join`` returns a dict of numpy arrays with the field names of
JoinOutput (None where the join has no such field); ``assert_same``
compares a JoinOutput (numpy or torch fields) against it, exactly and in
order."""

import numpy as np

FIELDS = ("keys", "a_vals", "b_vals", "a_valid", "b_valid", "a_idx", "b_idx")


def _positions(keys):
    pos = {}
    for i, k in enumerate(keys):
        pos.setdefault(k, []).append(i)
    return pos


def loop_join(a_keys, a_vals, b_keys, b_vals, how, indices=False):
    A = [int(k) for k in np.asarray(a_keys).view(np.uint64)]
    B = [int(k) for k in np.asarray(b_keys).view(np.uint64)]
    in_a, in_b = _positions(A), _positions(B)
    rows = []                                   # (key, a row or -1, b row or -1)
    if how == "right_outer":
        for j, k in enumerate(B):
            for i in in_a.get(k, [-1]):
                rows.append((k, i, j))
    else:
        for i, k in enumerate(A):
            hits = in_b.get(k, [])
            if how == "inner":
                rows.extend((k, i, j) for j in hits)
            elif how in ("left_outer", "full_outer"):
                rows.extend((k, i, j) for j in (hits or [-1]))
            elif how == "left_semi":
                if hits:
                    rows.append((k, i, -1))
            elif how == "left_anti":
                if not hits:
                    rows.append((k, i, -1))
            else:
                raise AssertionError(how)
        if how == "full_outer":
            rows.extend((k, -1, j) for j, k in enumerate(B) if k not in in_a)
    keys = np.array([r[0] for r in rows], dtype=np.uint64)
    a_idx = np.array([r[1] for r in rows], dtype=np.int64)
    b_idx = np.array([r[2] for r in rows], dtype=np.int64)

    def take(vals, idx):
        if vals is None:
            return None
        vals = np.asarray(vals).view(np.uint64)
        return np.array([int(vals[i]) if i >= 0 else 0 for i in idx],
                        dtype=np.uint64)

    one_sided = how in ("left_semi", "left_anti")
    return {
        "keys": keys,
        "a_vals": take(a_vals, a_idx),
        "b_vals": None if one_sided else take(b_vals, b_idx),
        "a_valid": a_idx >= 0,
        "b_valid": None if one_sided else b_idx >= 0,
        "a_idx": a_idx if indices else None,
        "b_idx": b_idx if indices and not one_sided else None,
    }


def as_dict(out):
    """A JoinOutput as the dict loop_join returns."""
    return {f: getattr(out, f) for f in FIELDS}


def _np(x):
    if x is None or isinstance(x, np.ndarray):
        return x
    return x.cpu().numpy()                      # torch tensor


def assert_same(got, want, what=""):
    """Every field equal, order included; u64 payloads compare by bits."""
    got = as_dict(got) if not isinstance(got, dict) else got
    want = as_dict(want) if not isinstance(want, dict) else want
    for f in FIELDS:
        g, w = _np(got[f]), _np(want[f])
        assert (g is None) == (w is None), f"{what} {f}: None mismatch"
        if g is None:
            continue
        if f in ("a_valid", "b_valid"):
            assert g.dtype == np.bool_, f"{what} {f}: dtype {g.dtype}"
        elif f in ("a_idx", "b_idx"):
            assert g.dtype == np.int64, f"{what} {f}: dtype {g.dtype}"
        else:
            assert g.dtype.itemsize == 8, f"{what} {f}: dtype {g.dtype}"
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert g.shape == w.shape, f"{what} {f}: {g.shape} != {w.shape}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (f"{what} {f}: {bad.size} rows differ, first "
                               f"at {bad[:1]}: {g[bad[:1]]} != {w[bad[:1]]}")
