"""urcco_dev_quota_cut on one GPU: a user_recommendations-shaped table of 1M rows x 128 results over a 200K-item catalogue, one rule (a brand per item,
max = 2), num = 20 -- and the only route there was before it: the table and the property's CSR copied to the host and the greedy run there in numpy.
HIP events, two warm-ups, five repetitions for the device; the wall clock, copies included, for the host.
Usage: python tools/quota_bench.py [LOG]   (profiles/quota_first_run.log is one run of it)"""
import os, sys, statistics, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from universal_recommender_amd import _lib
from universal_recommender_amd.device import DeviceSession

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
def say(*a):
    print(*a)
    if out:
        print(*a, file=out); out.flush()

dev = torch.device("cuda", 0)
sess = DeviceSession(dev, _lib.load(_lib.DEFAULT_PATH))
g = torch.Generator(device=dev); g.manual_seed(1)
N_ITEMS, N_ROWS, WIDTH, NUM, BRANDS, MOST = 200_000, 1_000_000, 128, 20, 200, 2

base = torch.randint(0, N_ITEMS, (N_ROWS, 1), device=dev, generator=g)
step = torch.randint(1, N_ITEMS // WIDTH, (N_ROWS, 1), device=dev, generator=g)
idx = ((base + step * torch.arange(WIDTH, device=dev)[None, :]) % N_ITEMS).to(torch.int32).contiguous()      # distinct inside a row
score = torch.sort(torch.rand((N_ROWS, WIDTH), dtype=torch.float64, device=dev, generator=g), dim=1, descending=True).values.contiguous()
count = torch.full((N_ROWS,), WIDTH, dtype=torch.int32, device=dev)
brand = torch.randint(0, BRANDS, (N_ITEMS,), device=dev, generator=g).to(torch.int32)                           # every item holds one value
row_ptr = torch.arange(N_ITEMS + 1, dtype=torch.int64, device=dev)
say(f"workload: {N_ROWS} rows x {WIDTH} results (full rows, distinct items), catalogue {N_ITEMS} items, one rule: {BRANDS} brands (uniform), one per item, max {MOST}, num {NUM}")

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

c, i, s, sh, st = timed(lambda: sess.quota_cut(count, idx, score, [(row_ptr, brand, MOST)], NUM, N_ITEMS), "urcco_dev_quota_cut (plan, its one synchronisation, both tiers)")
say("stats [lds rows, global rows, examined, rejected, resolve iterations, short rows]:", st.cpu().numpy()[:6].tolist(), " counts min/max:", int(c.min()), int(c.max()))

def host_route(chunk=65536):
    """every item holds one value, so a candidate is kept iff fewer than MOST earlier candidates of its row share its brand: the walk as array operations"""
    h_idx, h_score, h_brand = idx.cpu().numpy(), score.cpu().numpy(), brand.cpu().numpy()
    o_idx, o_score = np.full((N_ROWS, NUM), -1, np.int32), np.zeros((N_ROWS, NUM))
    for lo in range(0, N_ROWS, chunk):
        b = h_brand[h_idx[lo:lo + chunk]]
        order = np.argsort(b, axis=1, kind="stable")
        sb = np.take_along_axis(b, order, 1)
        start = np.concatenate([np.ones((len(b), 1), bool), sb[:, 1:] != sb[:, :-1]], 1)
        pos = np.arange(WIDTH)[None, :]
        nth = pos - np.maximum.accumulate(np.where(start, pos, 0), 1)                        # how many earlier candidates share the brand
        keep = np.empty_like(start)
        np.put_along_axis(keep, order, nth < MOST, 1)
        slot = np.cumsum(keep, 1) - 1
        r, j = np.nonzero(keep & (slot < NUM))
        o_idx[lo + r, slot[r, j]], o_score[lo + r, slot[r, j]] = h_idx[lo + r, j], h_score[lo + r, j]
    return o_idx, o_score

secs = []
for _ in range(3):
    t0 = time.perf_counter(); h_i, h_s = host_route(); secs.append(time.perf_counter() - t0)
say(f"the route before this call: table and property copied to the host, the greedy there in numpy: median {statistics.median(secs) * 1e3:.1f} ms, "
    f"min {min(secs) * 1e3:.1f}, max {max(secs) * 1e3:.1f}  (3 repetitions, wall clock, copies included)")
say("device == host, ids and score bits:", bool(np.array_equal(i.cpu().numpy(), h_i) and np.array_equal(s.cpu().numpy().view(np.int64), h_s.view(np.int64))))
sess.close()
