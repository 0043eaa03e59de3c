"""urcco_dev_diversify (decision D36) on one GPU: user_recommendations-shaped tables of 200K rows x 256 and 1M rows x 80 with Zipf-distributed items from a
200K-item catalogue, indicator rows of k = 50 (the tables of tools/list_metrics_bench.py), num = 20, penalty 0.25 -- the call alone, next to
urcco_dev_list_links on the same table (the same walk: the difference is the adjacency stores and the selection), and against a plain torch route on the same
device over as many rows as that route can afford: a padded gather-and-compare adjacency, a target position at a time, then num masked argmax steps.  HIP
events, two warm-ups, five repetitions; ids and score bits of both routes are compared.
Usage: python tools/diversify_bench.py [LOG] [--small]   (profiles/diversify_first_run.log is one run of it; --small: a rehearsal size)"""
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
N_ITEMS, K, NUM, PENALTY = (2_000, 50, 20, 0.25) if SMALL else (200_000, 50, 20, 0.25)
SHAPES = [(600, 256, 200), (3_000, 80, 300)] if SMALL else [(200_000, 256, 4_096), (1_000_000, 80, 16_384)]            # rows, width, the torch route's rows

zipf = 1.0 / torch.arange(1, N_ITEMS + 1, dtype=torch.float64, device=dev)
sim_rp = torch.arange(N_ITEMS + 1, dtype=torch.int64, device=dev) * K
sim_ci = torch.multinomial(zipf, N_ITEMS * K, replacement=True, generator=g).to(torch.int32).contiguous()
say(f"catalogue {N_ITEMS} items; similarity CSR: {K} entries a row, Zipf(1) columns; num {NUM}, penalty {PENALTY}")

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

for n, width, n_t in SHAPES:
    idx = torch.multinomial(zipf, n * width, replacement=True, generator=g).to(torch.int32).view(n, width).contiguous()   # head-heavy; an item may repeat in a row
    score = torch.sort(torch.rand((n, width), dtype=torch.float64, device=dev, generator=g), dim=1, descending=True).values.contiguous()
    count = torch.full((n,), width, dtype=torch.int32, device=dev)
    say(f"table {n} rows x {width}")
    d = timed(lambda: sess.diversify(count, idx, score, sim_rp, sim_ci, PENALTY, NUM, N_ITEMS, stats=True), "urcco_dev_diversify (statistics included)")
    timed(lambda: sess.list_links(count, idx, sim_rp, sim_ci, (width,), N_ITEMS), "urcco_dev_list_links on the same table, one cut-off = the width (zeroing the sums included)")
    timed(lambda: sess.diversify(count[:n_t], idx[:n_t], score[:n_t], sim_rp, sim_ci, PENALTY, NUM, N_ITEMS), f"urcco_dev_diversify over the first {n_t} rows")
    rows, walked, pairs, prefix = d[5].cpu().tolist()[:4]
    say(f"  stats: rows {rows}, matrix entries walked {walked} ({walked / max(rows, 1):.0f} a row), linked pairs {pairs} ({pairs / max(rows, 1):.1f} a row), rows left as their prefix {prefix}")

    def torch_route(chunk=1024):
        """first positions by a stable sort per row; adj[c, a, b] = some entry of a's matrix row is b's item, one b at a time, made symmetric; then NUM steps
        of key = score - w * links, the largest key at the smallest position"""
        o_idx, o_score = torch.full((n_t, NUM), -1, dtype=torch.int32, device=dev), torch.zeros((n_t, NUM), dtype=torch.float64, device=dev)
        pos = torch.arange(width, device=dev)
        for lo in range(0, n_t, chunk):
            r, s = idx[lo:min(lo + chunk, n_t)].long(), score[lo:min(lo + chunk, n_t)]
            c = torch.arange(r.shape[0], device=dev)
            srt, order = torch.sort(r, dim=1, stable=True)
            rep = torch.zeros_like(r, dtype=torch.bool)
            rep.scatter_(1, order[:, 1:], srt[:, 1:] == srt[:, :-1])                                                       # a later repeat of an item
            ent = sim_ci.view(N_ITEMS, K)[r].long()                                                                         # [c, width, K]
            adj = torch.zeros((r.shape[0], width, width), dtype=torch.bool, device=dev)
            for b in range(width):
                adj[:, :, b] = (ent == r[:, b, None, None]).any(2) & (r != r[:, b, None]) & ~rep & ~rep[:, b, None]
            adj |= adj.transpose(1, 2).clone()
            top = torch.where(rep, -torch.inf, s).max(1).values
            w = torch.where(top > 0, PENALTY * top, 0.0)
            links, alive = torch.zeros_like(s), ~rep
            for t in range(NUM):
                key = torch.where(alive, s - w[:, None] * links, -torch.inf)
                e = torch.where(key == key.max(1, keepdim=True).values, pos, width).min(1).values                          # the smallest position of the largest key
                ok = alive[c, e]
                o_idx[lo:lo + chunk, t] = torch.where(ok, r[c, e], -1).int()
                o_score[lo:lo + chunk, t] = torch.where(ok, s[c, e], 0.0)
                alive[c, e] = False
                links += adj[c, e]
        return o_idx, o_score
    t_idx, t_score = timed(torch_route, f"torch: padded gather-and-compare adjacency + {NUM} masked argmax steps over {n_t} rows", warm=1, reps=2)
    say(f"  device == torch over those rows (ids, score bits): {bool((d[1][:n_t] == t_idx).all())}, {bool((d[2][:n_t].view(torch.int64) == t_score.view(torch.int64)).all())}")
sess.close()
