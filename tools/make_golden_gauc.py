#!/usr/bin/env python
"""Writes tests/golden/g18_gauc.npz: the reference's gauc_score (base.py:33-64 — sklearn's roc_auc_score per user) on a small
evaluation set, over the whole set and per domain, with weights=None (the user's row count) and with a dict of non-integer
weights.  gauc_score is imported from the reference checkout (CDC_REFERENCE, as tools/make_golden.py); nothing of it is copied.

The set: the 500 scores of g9_metrics.npz (rounded to two decimals: ties), 4 domains, 42 users; user 40 has one row, user 41 has
several rows of one class, two users hold -0.0 and +0.0 under different labels, and every row of domain 3 is positive, so no
user of domain 3 can be counted — gauc_score divides by zero there, recorded as NaN.

The archive is written with fixed member dates, so a rerun reproduces the file bit for bit.
"""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, SEED  # noqa: E402


def save_npz_reproducibly(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    if not os.path.isdir(REF):
        sys.exit(f"reference not mounted at {REF}; golden vectors can only be regenerated in the build container")
    sys.path.insert(0, REF)
    from base import gauc_score

    n, n_domain, n_user = 500, 4, 42
    rng = np.random.default_rng(SEED + 18)
    s = np.load(os.path.join(OUT, "g9_metrics.npz"))["scores"].astype(np.float32).copy()
    assert s.shape == (n,)
    t = rng.integers(0, 2, size=n).astype(np.int64)
    u = rng.integers(0, 40, size=n).astype(np.int64)
    dom = rng.integers(0, n_domain, size=n).astype(np.int64)
    # signed zeros that must tie: user 7 (domain 0) and user 11 (domain 1) each get -0.0 and +0.0 under different labels
    for k, (usr, d) in enumerate([(7, 0), (11, 1)]):
        i = 20 * k
        u[i:i + 4], dom[i:i + 4] = usr, d
        s[i:i + 4] = [-0.0, 0.0, 0.0, -0.0]
        t[i:i + 4] = [1, 0, 1, 0]
    u[100], dom[100] = 40, 2                                       # a user with one row
    u[101:106], dom[101:106], t[101:106] = 41, [0, 0, 1, 2, 2], 0  # a user with one class only
    t[dom == 3] = 1                                                # a domain with no countable user
    w = 0.25 + 3.0 * rng.random(n_user)                            # non-integer weights
    wdict = {int(k): float(w[k]) for k in range(n_user)}

    def ref(mask, weights):
        try:
            return float(gauc_score([int(v) for v in t[mask]], [float(v) for v in s[mask]], [int(v) for v in u[mask]], weights))
        except ZeroDivisionError:                                   # no user with both classes: score / num with num == 0
            return float("nan")

    arrays = {"scores": s, "targets": t, "users": u, "domains": dom, "weights": w,
              "n_user": np.array(n_user), "n_domain": np.array(n_domain)}
    everything = np.ones(n, dtype=bool)
    arrays["gauc_all_none"] = np.array(ref(everything, None))
    arrays["gauc_all_w"] = np.array(ref(everything, wdict))
    for d in range(n_domain):
        arrays[f"gauc_d{d}_none"] = np.array(ref(dom == d, None))
        arrays[f"gauc_d{d}_w"] = np.array(ref(dom == d, wdict))
    path = os.path.join(OUT, "g18_gauc.npz")
    save_npz_reproducibly(path, arrays)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays)")
    for k in sorted(arrays):
        if k.startswith("gauc_"):
            print(f"  {k} = {float(arrays[k])!r}")


if __name__ == "__main__":
    main()
