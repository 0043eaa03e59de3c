"""The list metrics of decision D35 on one GPU: urcco_dev_list_exposure, urcco_dev_exposure_stats and urcco_dev_list_links over user_recommendations-shaped
tables of 1M rows x 20 and 200K rows x 256 with Zipf-distributed items from a 200K-item catalogue and indicator rows of k = 50, each against a plain torch
route on the same device: bincount for the histogram, sort + cumsum for R, a padded gather-and-compare for the links.  HIP events, two warm-ups, five
repetitions; the integers of both routes are compared.
Usage: python tools/list_metrics_bench.py [LOG] [--small]   (profiles/list_metrics_first_run.log is one run of it; --small: a rehearsal size)"""
import os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from universal_recommender_amd import _lib
from universal_recommender_amd.device import DeviceSession

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out = open(args[0], "w") if args else None
def say(*a):
    print(*a)
    if out:
        print(*a, file=out); out.flush()

dev = torch.device("cuda", 0)
sess = DeviceSession(dev, _lib.load(_lib.DEFAULT_PATH))
g = torch.Generator(device=dev); g.manual_seed(1)
SMALL = "--small" in sys.argv
N_ITEMS, K = (2_000, 50) if SMALL else (200_000, 50)
SHAPES = [(3_000, 20, (1, 5, 10, 20)), (500, 256, (10, 50, 100, 256))] if SMALL else [(1_000_000, 20, (1, 5, 10, 20)), (200_000, 256, (10, 50, 100, 256))]

zipf = 1.0 / torch.arange(1, N_ITEMS + 1, dtype=torch.float64, device=dev)
sim_rp = torch.arange(N_ITEMS + 1, dtype=torch.int64, device=dev) * K
sim_ci = torch.multinomial(zipf, N_ITEMS * K, replacement=True, generator=g).to(torch.int32).contiguous()          # an entry may repeat: both routes count it each time
say(f"catalogue {N_ITEMS} items; similarity CSR: {K} entries a row, Zipf(1) columns")

def timed(fn, label, warm=2, reps=5):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    say(f"  {label}: median {statistics.median(ms):.3f} ms, min {min(ms):.3f}, max {max(ms):.3f}  ({warm} warm-ups, {reps} repetitions, HIP events)")
    return r

for n, num, ks in SHAPES:
    idx = torch.multinomial(zipf, n * num, replacement=True, generator=g).to(torch.int32).view(n, num).contiguous()     # head-heavy; an item may repeat in a row
    count = torch.full((n,), num, dtype=torch.int32, device=dev)
    kt = torch.tensor(ks, device=dev)
    say(f"table {n} rows x {num}, ks = {list(ks)}")
    bucket = timed(lambda: sess.list_exposure(count, idx, ks, N_ITEMS), "urcco_dev_list_exposure (zeroing the histogram included)")

    def torch_exposure():
        x = torch.bucketize(torch.arange(num, device=dev), kt, right=True)                                              # x(j) per position
        return torch.bincount((x[None, :] * N_ITEMS + idx).reshape(-1), minlength=len(ks) * N_ITEMS).view(len(ks), N_ITEMS)
    t_bucket = timed(torch_exposure, "torch: bucketize + bincount")
    expo, stats = timed(lambda: sess.exposure_stats(bucket), "urcco_dev_exposure_stats (running sums, three reductions, one radix sort and rank sum per cut-off)")

    def torch_stats():
        e = torch.cumsum(t_bucket, 0)
        rank = torch.arange(1, N_ITEMS + 1, device=dev)
        return e, torch.stack([(e > 0).sum(1), e.sum(1), (e * e).sum(1), (torch.sort(e, 1).values * rank[None, :]).sum(1)], 1)
    t_expo, t_stats = timed(torch_stats, "torch: cumsum + sort + sums")
    linked, _ = timed(lambda: sess.list_links(count, idx, sim_rp, sim_ci, ks, N_ITEMS), "urcco_dev_list_links (zeroing the sums included)")
    n_t = min(n, 20_000) if num > 64 else n                                                                                # the torch route's rows: the wide table in full takes minutes
    if n_t < n:
        timed(lambda: sess.list_links(count[:n_t], idx[:n_t], sim_rp, sim_ci, ks, N_ITEMS), f"urcco_dev_list_links over the first {n_t} rows")

    def torch_links(chunk=2048 if num > 64 else 65536):
        """first positions by a stable sort per row, then every entry of every listed item's similarity row compared with the row: [chunk, num, K, num] booleans"""
        res = torch.empty((n_t, len(ks)), dtype=torch.int64, device=dev)
        pos = torch.arange(num, device=dev)
        for lo in range(0, n_t, chunk):
            r = idx[lo:min(lo + chunk, n_t)].long()
            srt, order = torch.sort(r, dim=1, stable=True)
            rep = torch.zeros_like(r, dtype=torch.bool)
            rep.scatter_(1, order[:, 1:], srt[:, 1:] == srt[:, :-1])                                                      # a later repeat of an item
            ent = sim_ci.view(N_ITEMS, K)[r].long()                                                                        # [c, num, K]
            acc = torch.zeros((r.shape[0], len(ks)), dtype=torch.int64, device=dev)
            for b in range(num):                                                                                          # one target position at a time: memory
                hit = (ent == r[:, b, None, None]) & (ent != r[:, :, None]) & ~rep[:, :, None] & ~rep[:, b, None, None]     # [c, num(a), K]
                far = torch.maximum(pos[None, :], pos[b])                                                                  # [1, num(a)]
                acc += (hit.sum(2)[:, :, None] * (far[:, :, None] < kt[None, None, :])).sum(1)
            res[lo:lo + chunk] = acc
        return res
    t_linked = timed(torch_links, f"torch: padded gather-and-compare over {n_t} rows, a target position at a time", warm=1, reps=2 if num > 64 else 3)
    same = (bool((bucket.view(torch.int32) == t_bucket).all()), bool((expo == t_expo).all()), bool((stats == t_stats).all()), bool((linked[:n_t].long() == t_linked).all()))
    say(f"  device == torch (bucket, expo, stats, linked): {same};  covered {stats[:, 0].tolist()}, sum of linked {linked.sum(0).tolist()}")
sess.close()
