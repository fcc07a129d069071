"""rocprofv3 kernel trace (csv) of calls in flight: every kernel's time, the gaps on every hardware queue, what runs side by side --
and, with the library's call stamps of the same run (tools/cycle_stamps.py), where one call's cycle goes.

    python tools/inflight_timeline.py <kernel_trace.csv> [stamps.json]

On the lanes the kernels of one call sit on two queues (the transpose -- with a clear in front of it in traces of libraries whose
transposer does not empty the duplicate search's table itself -- on the transpose lane, the rest on the call's parse lane), so a call is
put together from the stamps: record `seq` is the call's place on the transpose lane (the n-th transpose there), `lane` its parse lane
(the calls of one lane, in seq order, are the key tables of one queue in start order).  Without clears in the trace "clear" below
reads "the call's first kernel": the transpose.  The cycle of a
call -- from its entry to the same thread's next entry -- is then split into

  d  entry -> first launch (d1: the poll of the caller's stream and the lane mutex, d2: lanes taken -> clear launched)
  f  the clear waits behind another call's transpose on the transpose lane
  e  launch (or the lane coming free) -> the clear's start on the device
  g  the key table waits on its parse lane behind the call that holds it (g_avoidable: the part another lane would have spared)
  a  the tail kernel's end -> the calling thread sees completion
  b  that -> return from the C call
  c  outside the library (return -> the thread's next entry)

and the kernels themselves with the small gaps between them."""
import collections
import csv
import json
import sys


def kind(n):
    return ("parse" if "lz4_chunks_kernel" in n else "transp" if "bitswap1_u16" in n else "key" if "dedupe_key" in n else
            "clear" if "dedupe_clear" in n else "tail" if "inplace_tail_fused" in n else "scan" if "frame_scan" in n else
            "stash" if "stash" in n else "gather" if "frame_gather" in n else "finish" if "inplace_finish" in n else
            "marks" if "tail_marks" in n else "other:" + n[:30])


def stats(v):
    v = sorted(v)
    n = len(v)
    if not n:
        return "n    0"
    mean = sum(v) / n
    sd = (sum((x - mean) ** 2 for x in v) / n) ** 0.5
    return "n %4d mean %7.1f sd %6.1f  p10 %7.1f p50 %7.1f p90 %7.1f max %7.1f" % (n, mean, sd, v[n // 10], v[n // 2], v[min(n - 1, 9 * n // 10)], v[-1])


def trace_summary(rows):
    parses = [r for r in rows if r[2] == "parse"]
    # the longest run of parses whose starts are less than 1.2 ms apart
    best, i = (0, 0), 0
    while i < len(parses):
        j = i
        while j + 1 < len(parses) and parses[j + 1][0] - parses[j][0] < 1_200_000:
            j += 1
        if j - i > best[1] - best[0]:
            best = (i, j)
        i = j + 1
    a, b = best
    if b - a < 20:
        print("too few parses in a row (%d)" % (b - a + 1))
        return
    t0, t1 = parses[a + 8][0], parses[b - 8][0]
    ncalls = b - 8 - (a + 8)
    print("window %.2f ms, %d parses -> %.4f ms/step" % ((t1 - t0) / 1e6, ncalls, (t1 - t0) / 1e6 / ncalls))
    win = [r for r in rows if r[0] >= t0 and r[1] <= t1]
    dur = collections.defaultdict(list)
    for s, e, n, q in win:
        dur[n].append((e - s) / 1e3)
    for n, v in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
        print("  %-10s n %4d mean %8.1f us  sum/step %.3f ms" % (n, len(v), sum(v) / len(v), sum(v) / 1e3 / ncalls))
    byq = collections.defaultdict(list)
    for r in win:
        byq[r[3]].append(r)
    gaps = collections.defaultdict(list)
    print("queues:")
    for q, v in sorted(byq.items()):
        v.sort()
        for x, y in zip(v, v[1:]):
            gaps[(x[2], y[2])].append((y[0] - x[1]) / 1e3)
        print("  queue %d: busy %5.1f %%  %s" % (q, 100.0 * sum(e - s for s, e, _, _ in v) / (t1 - t0), dict(collections.Counter(r[2] for r in v))))
    print("gaps (end->start) per queue:")
    for k, v in sorted(gaps.items(), key=lambda kv: -sum(kv[1])):
        print("  %-8s -> %-8s n %4d mean %8.1f us  sum/step %.3f ms" % (k[0], k[1], len(v), sum(v) / len(v), sum(v) / 1e3 / ncalls))
    ev = []
    for s, e, n, q in win:
        if n in ("parse", "transp"):
            ev.append((s, 1, n))
            ev.append((e, -1, n))
    ev.sort()
    cnt, last, hist = {"parse": 0, "transp": 0}, t0, collections.Counter()
    for t, d, n in ev:
        hist[(cnt["transp"], cnt["parse"])] += t - last
        last = t
        cnt[n] += d
    tot = sum(hist.values())
    print("concurrency (transposes, parses): share")
    for k, v in sorted(hist.items(), key=lambda kv: -kv[1])[:12]:
        print("   T=%d P=%d : %5.1f %%" % (k[0], k[1], 100 * v / tot))


def calls_from_stamps(rows, st):
    """one dict per stamped call on the lanes: its stamps (steady-clock ns) and its kernels (device ns), or None where the trace and
    the stamps do not fit together"""
    f = st["fields"]
    recs = sorted((dict(zip(f, r)) for r in st["stamps"] if r[f.index("seq")] >= 0), key=lambda r: r["seq"])
    n = len(recs)
    print("stamps: %d calls (%d on the lanes), %.4f ms/step by the wall clock" % (len(st["stamps"]), n, st["ms_per_step"]))
    if n < 8:
        return None
    byk = collections.defaultdict(list)
    for r in rows:
        byk[r[2]].append(r)
    # the transpose lane's queue: where the last n transposes are
    tq = collections.Counter(r[3] for r in byk["transp"][-n:]).most_common(1)[0][0]
    transps = [r for r in byk["transp"] if r[3] == tq][-n:]
    clears = [r for r in byk["clear"] if r[3] == tq][-n:]
    if not clears:
        print("  no clear on the transpose lane: a call's first kernel is its transpose")
        clears = [(t[0], t[0], "clear", t[3]) for t in transps]
    if len(clears) < n or len(transps) < n:
        print("the trace holds %d clears and %d transposes on queue %d, the stamps %d calls: no attribution" % (len(clears), len(transps), tq, n))
        return None
    for r, c, t in zip(recs, clears, transps):
        r["clear"], r["transp"] = c, t
    # a lane's queue: the one whose last key tables all start behind the transposes of the lane's calls
    bylane = collections.defaultdict(list)
    for r in recs:
        bylane[r["lane"]].append(r)
    keyq = collections.defaultdict(list)
    for r in byk["key"]:
        keyq[r[3]].append(r)
    used = set()
    for lane, lr in sorted(bylane.items()):
        best = None
        for q, ks in keyq.items():
            if q in used or len(ks) < len(lr):
                continue
            ks = ks[-len(lr):]
            slack = [k[0] - r["transp"][1] for r, k in zip(lr, ks)]
            if min(slack) >= 0 and (best is None or sum(slack) < best[0]):
                best = (sum(slack), q)
        if best is None:
            print("no queue fits the %d calls of parse lane %d: no attribution" % (len(lr), lane))
            return None
        q = best[1]
        used.add(q)
        on_q = {k: [x for x in byk[k] if x[3] == q][-len(lr):] for k in ("key", "parse", "tail")}
        if min(len(v) for v in on_q.values()) < len(lr):
            print("queue %d lacks kernels for parse lane %d: no attribution" % (q, lane))
            return None
        for i, r in enumerate(lr):
            r["key"], r["parse"], r["tail"], r["queue"] = on_q["key"][i], on_q["parse"][i], on_q["tail"][i], q
        print("  parse lane %d: queue %d, %d calls" % (lane, q, len(lr)))
    print("  transpose lane: queue %d" % tq)
    # the device's clock against the steady clock: the clock under which a clear starts soonest behind its launch, but never before it
    base = st["clocks_ns"]["CLOCK_MONOTONIC"]
    pick = None
    for name, v in st["clocks_ns"].items():
        lat = min(r["clear"][0] - (v - base) - r["clear_launched"] for r in recs)
        if 0 <= lat < 5_000_000 and (pick is None or lat < pick[1]):
            pick = (name, lat, v - base)
    if pick is None:
        off = min(r["clear"][0] - r["clear_launched"] for r in recs) - 5000
        print("  device clock: none of %s fits; calibrated so that the quickest clear starts 5 us behind its launch (a, e relative to that)" % sorted(st["clocks_ns"]))
    else:
        off = pick[2]
        print("  device clock: %s (the quickest clear starts %.1f us behind its launch)" % (pick[0], pick[1] / 1e3))
    for r in recs:
        for k in ("clear", "transp", "key", "parse", "tail"):
            r[k] = (r[k][0] - off, r[k][1] - off)
    return recs


def cycle_split(recs):
    bythread = collections.defaultdict(list)
    for r in recs:
        bythread[r["thread"]].append(r)
    for v in bythread.values():
        v.sort(key=lambda r: r["entry"])
        for x, y in zip(v, v[1:]):
            x["next_entry"] = y["entry"]
    lanes = sorted(set(r["lane"] for r in recs))
    terms = collections.defaultdict(list)
    lat = []
    for i, r in enumerate(recs):
        if "next_entry" not in r or i == 0:
            continue
        prev_t_end = recs[i - 1]["transp"][1]
        # when the lanes come free of the calls in front of this one
        free = {l: max([x["tail"][1] for x in recs[:i] if x["lane"] == l] or [0]) for l in lanes}
        t_end = r["transp"][1]
        own = max(t_end, free[r["lane"]])
        alt = min(max(t_end, free[l]) for l in lanes)
        us = lambda x: x / 1e3
        row = {
            "d1 entry -> lanes taken": us(r["lanes_taken"] - r["entry"]),
            "d2 lanes taken -> clear launched": us(r["clear_launched"] - r["lanes_taken"]),
            "f  behind another call's transpose": us(max(0, prev_t_end - r["clear_launched"])),
            "e  launch / lane free -> clear starts": us(r["clear"][0] - max(r["clear_launched"], prev_t_end)),
            "   clear + transpose (kernels, gap)": us(r["transp"][1] - r["clear"][0]),
            "g  behind the parse lane's holder": us(own - t_end),
            "   g avoidable (another lane free earlier)": us(own - alt),
            "   lane free -> key table starts": us(r["key"][0] - own),
            "   key + parse + tail (kernels, gaps)": us(r["tail"][1] - r["key"][0]),
            "a  tail ends -> thread sees completion": us(r["sync_returned"] - r["tail"][1]),
            "b  -> return from the C call": us(r["returned"] - r["sync_returned"]),
            "c  outside the library": us(r["next_entry"] - r["returned"]),
            "cycle (entry -> the thread's next entry)": us(r["next_entry"] - r["entry"]),
            "   host: clear launched -> all queued": us(r["parse_queued"] - r["clear_launched"]),
        }
        for k, v in row.items():
            terms[k].append(v)
        lat.append(us(r["tail"][1] - r["clear"][0]))
    print("one call's cycle, microseconds (calls with a successor on their thread):")
    for k, v in terms.items():
        print("  %-44s %s" % (k, stats(v)))
    print("  %-44s %s" % ("call latency clear -> tail end", stats(lat)))
    agg = lambda k: sum(terms[k]) / max(1, len(terms[k]))
    waits = sum(agg(k) for k in terms if k[0] in "abcdefg" and k[1] in " 12" and not k.startswith("cycle"))
    print("  a + b + c + d + e + f + g = %.1f us of a cycle of %.1f us (%.1f %%)" % (waits, agg("cycle (entry -> the thread's next entry)"),
                                                                             100 * waits / max(1e-9, agg("cycle (entry -> the thread's next entry)"))))


def main():
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind(r["Kernel_Name"]), int(r["Queue_Id"])) for r in csv.DictReader(open(sys.argv[1])))
    trace_summary(rows)
    if len(sys.argv) > 2:
        recs = calls_from_stamps(rows, json.load(open(sys.argv[2])))
        if recs:
            cycle_split(recs)


if __name__ == "__main__":
    main()
