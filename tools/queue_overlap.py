"""rocprofv3 kernel trace (csv) of the in-flight bench: which hardware queue the kernels ran on and what overlapped.

    python tools/queue_overlap.py <kernel_trace.csv>

Per queue: kernels by kind and busy share of the steady window; per pair of queues: time kernels of both ran side by side; for
the transposes: the gap to the kernel in front on the same queue, split by what that kernel was (a parse in front of a transpose
on the same queue is another call's: a call's own parse runs behind its transpose)."""
import collections
import csv
import sys


def kind(n):
    return ("parse" if "lz4_chunks_kernel" in n else "transp" if "bitswap1_u16" in n else "key" if "dedupe_key" in n else
            "clear" if "dedupe_clear" in n else "tail" if "inplace_tail_fused" in n else "other")


def main(path):
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind(r["Kernel_Name"]), int(r["Queue_Id"]))
                  for r in csv.DictReader(open(path)))
    parses = [r for r in rows if r[2] == "parse"]
    if len(parses) < 40:
        print("too few parses (%d)" % len(parses))
        return
    # steady window: the middle half of the parses
    t0, t1 = parses[len(parses) // 4][0], parses[3 * len(parses) // 4][0]
    win = [r for r in rows if r[0] >= t0 and r[1] <= t1]
    ncalls = sum(1 for r in win if r[2] == "parse")
    print("window %.2f ms, %d parses -> %.4f ms/step" % ((t1 - t0) / 1e6, ncalls, (t1 - t0) / 1e6 / ncalls))
    byq = collections.defaultdict(list)
    for r in win:
        byq[r[3]].append(r)
    print("queues in use: %d" % len(byq))
    for q, v in sorted(byq.items()):
        c = collections.Counter(r[2] for r in v)
        busy = sum(e - s for s, e, _, _ in v)
        print("  queue %d: busy %5.1f %%  %s" % (q, 100.0 * busy / (t1 - t0), dict(c)))
    # side by side, per pair of queues (only parse and transpose: the long kernels)
    long_k = {q: [(s, e) for s, e, n, _ in v if n in ("parse", "transp")] for q, v in byq.items()}
    qs = sorted(long_k)
    print("parse/transpose kernels of two queues side by side (share of the window):")
    for i, a in enumerate(qs):
        for b in qs[i + 1:]:
            ov, j = 0, 0
            for s, e in long_k[a]:
                while j < len(long_k[b]) and long_k[b][j][1] <= s:
                    j += 1
                k = j
                while k < len(long_k[b]) and long_k[b][k][0] < e:
                    ov += min(e, long_k[b][k][1]) - max(s, long_k[b][k][0])
                    k += 1
            print("  queues %d,%d: %5.1f %%" % (a, b, 100.0 * ov / (t1 - t0)))
    # what a transpose follows on its queue
    front = collections.defaultdict(list)
    for q, v in byq.items():
        for x, y in zip(v, v[1:]):
            if y[2] == "transp":
                # (a clear sits between: look through it)
                front[x[2]].append((y[0] - x[1]) / 1e3)
        for w, x, y in zip(v, v[1:], v[2:]):
            if y[2] == "transp" and x[2] == "clear":
                front["clear<-" + w[2]].append((x[0] - w[1]) / 1e3)
    print("kernel in front of a transpose on its queue: n, mean gap (us)")
    for k, g in sorted(front.items()):
        print("  %-14s n %4d  gap %8.1f" % (k, len(g), sum(g) / len(g)))
    # transposes: share of the window one runs, parses side by side
    ev = []
    for s, e, n, _ in win:
        if n in ("parse", "transp"):
            ev += [(s, 1, n), (e, -1, n)]
    ev.sort()
    cnt, last, hist = {"parse": 0, "transp": 0}, t0, collections.Counter()
    for t, d, n in ev:
        hist[(min(cnt["transp"], 1), cnt["parse"])] += t - last
        last = t
        cnt[n] += d
    tot = float(sum(hist.values()))
    print("a transpose runs: %.1f %% of the window" % (100 * sum(v for k, v in hist.items() if k[0]) / tot))
    for p in range(0, 6):
        share = sum(v for k, v in hist.items() if k[1] == p) / tot
        if share > 0.001:
            print("  %d parses side by side: %5.1f %%" % (p, 100 * share))


if __name__ == "__main__":
    main(sys.argv[1])
