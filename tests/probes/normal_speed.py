"""Cost of alg_kkt_normal_equations on the C2 shape (3-player DoubleIntegrator, N = 40, 4096 games, after one solve).

    python tests/probes/normal_speed.py [--games 4096] [--rounds 7] [--out FILE]

wrt = ("xf", "Q"): 24 columns.  Two routes to the same H, g and loss, alternated in one process after a warm-up of each, host clock around
synchronous calls, median over the rounds and every round's figure:
  new      one Batch.kkt_normal_equations call: upload of target and weight, two k_kkt_sens launches, one k_sens_gram launch, download of
           H, g, loss and status
  parent   what the commit before the entry point offers: two Batch.kkt_sensitivity calls (all columns downloaded), then numpy Gram
           products on the host (batched matmul)
The floor of k_sens_gram is the column scratch read once over the HBM bandwidth; its own time comes from a kernel trace of this probe
(rocprofv3 --kernel-trace --stats), not from here."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import algames_jl_amd as alg  # noqa: E402

HBM = 6.3e12          # achievable bytes / s of the MI355X's HBM


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    outs = [sys.stdout]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        outs.append(open(a.out, "a"))

    def say(s):
        for f in outs:
            print(s, file=f, flush=True)
    B = a.games
    prob = alg.scenarios.make_problem("C2", np.arange(B))
    b = prob.batch
    alg.newton_solve(prob)
    cols = alg.normal_columns(b, ("xf", "Q"))
    q = len(cols)
    z = b.get_traj()[:, b.n:]
    target = z + np.random.default_rng(0).uniform(-0.1, 0.1, z.shape)
    w = alg.default_fit_weight(b)
    say("# normal equations at C2 (%d games, N = %d, S = %d, q = %d columns)" % (B, b.N, b.S, q))

    def new():
        return b.kkt_normal_equations(cols, target, w)

    def parent():
        X = np.concatenate([b.kkt_sensitivity("xf")[0], b.kkt_sensitivity("Q")[0]], axis=1)       # (B, q, S)
        r = b.get_traj()[:, b.n:] - target
        Xw = X * w
        return Xw @ X.transpose(0, 2, 1), np.einsum("bqs,bs->bq", Xw, r), 0.5 * np.einsum("bs,s,bs->b", r, w, r)
    Hn, gn, ln, st = new()
    Hp, gp, lp = parent()
    assert np.all(st == 0)
    scale = np.abs(Hp).max(axis=(1, 2), keepdims=True)
    say("# the two routes agree: max |H_new - H_parent| / max |H| = %.2e, g %.2e, loss %.2e" % (
        (np.abs(Hn - Hp) / scale).max(), (np.abs(gn - gp) / np.abs(gp).max(axis=1, keepdims=True)).max(), (np.abs(ln - lp) / lp).max()))
    t = {"new": [], "parent": []}
    for _ in range(a.rounds):
        for name, fn in (("new", new), ("parent", parent)):
            t0 = time.perf_counter()
            fn()
            t[name].append(1e3 * (time.perf_counter() - t0))
    for name in ("new", "parent"):
        say("%-8s median %9.2f ms   rounds %s" % (name, np.median(t[name]), " ".join("%.2f" % v for v in t[name])))
    say("# parent / new = %.1f x" % (np.median(t["parent"]) / np.median(t["new"])))
    scratch = 8.0 * B * q * b.S
    say("# column scratch %.0f MB: read once at %.1f TB/s = %.3f ms, the floor of k_sens_gram; downloads: new %.1f MB, parent %.0f MB" % (
        scratch / 1e6, HBM / 1e12, 1e3 * scratch / HBM, (Hn.nbytes + gn.nbytes + ln.nbytes + st.nbytes) / 1e6, scratch / 1e6))


if __name__ == "__main__":
    main()
