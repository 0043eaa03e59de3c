"""urcco_dev_audience on one GPU: 64 query items over 1M users' term rows on a 200K-item model -- all users in one call, in chunks of 65 536, and the route
that existed before it (urcco_dev_recommend(num = 256) over the same users and a search of the rows).  HIP events, two warm-ups, five repetitions.
Usage: python tools/audience_bench.py [LOG]   (profiles/audience_first_run.log is one run of it)"""
import os, sys, statistics
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from universal_recommender_amd import _lib
from universal_recommender_amd.device import DeviceSession, DevCsr

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
def say(*a):
    print(*a)
    if out:
        print(*a, file=out); out.flush()

dev = torch.device("cuda", 0)
sess = DeviceSession(dev, _lib.load(_lib.DEFAULT_PATH))
g = torch.Generator(device=dev); g.manual_seed(1)
N_ITEMS, N_USERS, K, T, NQ, NUM = 200_000, 1_000_000, 50, 20, 64, 100

def rows(n_rows, width, n_cols, sort):
    base = torch.randint(0, n_cols, (n_rows, 1), device=dev, generator=g)
    step = torch.randint(1, n_cols // width, (n_rows, 1), device=dev, generator=g)
    c = (base + step * torch.arange(width, device=dev)[None, :]) % n_cols       # distinct inside a row
    if sort:
        c = torch.sort(c, dim=1).values
    return torch.arange(0, (n_rows + 1) * width, width, dtype=torch.int64, device=dev), c.reshape(-1).to(torch.int32).contiguous()

i_rp, i_ci = rows(N_ITEMS, K, N_ITEMS, False)
u_rp, u_ci = rows(N_USERS, T, N_ITEMS, True)
items = torch.randint(0, N_ITEMS, (NQ,), device=dev, generator=g).to(torch.int32)
excl = (torch.zeros(N_USERS + 1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
say(f"workload: {NQ} query items, {N_USERS} users x {T} terms (uniform), model {N_ITEMS} items x {K} indicators (uniform), one clause, boost 1.0, num {NUM}")

def timed(fn, label, warm=2, reps=5):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    say(f"{label}: median {statistics.median(ms):.3f} ms, min {min(ms):.3f}, max {max(ms):.3f}  ({warm} warm-ups, {reps} repetitions, HIP events)")
    return r

clause = [(N_ITEMS, 1.0, i_rp, i_ci, u_rp, u_ci, None)]
def audience_once():
    return sess.audience(items, N_ITEMS, clause, NUM, N_USERS, None, excl)
c, u, s, st = timed(audience_once, "urcco_dev_audience, all users in one call")
say("stats [tiles, slabs, compactions, kept, overflows]:", st.cpu().numpy()[:5].tolist(), " audience sizes min/max:", int(c.min()), int(c.max()))

CH = 65536
def audience_chunked():
    o = None
    for lo in range(0, N_USERS, CH):
        hi = min(lo + CH, N_USERS)
        rp = (u_rp[lo:hi + 1] - u_rp[lo]).contiguous()
        o = sess.audience(items, N_ITEMS, [(N_ITEMS, 1.0, i_rp, i_ci, rp, u_ci[int(u_rp[lo]):], None)], NUM, hi - lo,
                          torch.arange(lo, hi, dtype=torch.int32, device=dev), (excl[0][: hi - lo + 1], excl[1]), o, stats=False)[:3]
    return o
c2, u2, s2 = timed(audience_chunked, f"urcco_dev_audience, chunks of {CH} users (row slicing included)")
say("chunked == one call, bit for bit:", bool(torch.equal(c, c2) and torch.equal(u, u2) and torch.equal(s, s2)))

nnz = int(i_rp[-1])
cp, ri = sess.transpose(DevCsr(N_ITEMS, N_ITEMS, i_rp, i_ci, nnz), sess.column_counts(i_ci, nnz, N_ITEMS))
def parent_route():
    found = 0
    for lo in range(0, N_USERS, CH):
        hi = min(lo + CH, N_USERS)
        rp = (u_rp[lo:hi + 1] - u_rp[lo]).contiguous()
        cnt, idx, sc, _ = sess.recommend(hi - lo, N_ITEMS, [(N_ITEMS, 1.0, cp, ri, rp, u_ci[int(u_rp[lo]):])], 256, None, None, None, _lib.REC_NO_BACKFILL, stats=False)
        found += int(torch.isin(idx, items).sum())
    return found
found = timed(parent_route, "the route before this call: urcco_dev_recommend(num = 256, no backfill) over the same users + a search of the rows for the items")
say(f"  (that route finds {found} (user, item) slots and does NOT return the same answer: an item outside a user's top 256 is lost, and no per-item top-{NUM} is cut)")
sess.close()
