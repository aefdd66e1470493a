"""The tail of the factorisation in a rocprofv3 kernel trace of tools/time_sizes.py (last step): the split of
tools/step_budget.py taken before / inside the last TAIL bulk launches, and per launch of the tail its HSA queue,
workgroups, duration and gap to the next one, with the block kernels (gpak_potrf128_f64 "8w" / gpak_potrf128_co_f64 "co")
and panel products that started while it ran.   python tools/tail_budget.py <kernel_trace.csv> [TAIL=24] [-v]"""
import csv, sys, collections
f = sys.argv[1]
NT = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 24
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
S = lambda r: int(r["Start_Timestamp"]); E = lambda r: int(r["End_Timestamp"])
isbulk = lambda r: "gemm_nt_f64_rs<4, 2, true" in r["Kernel_Name"]
names = collections.Counter(r["Kernel_Name"][:60] for r in rows)
if "-v" in sys.argv:
    for k, v in names.most_common(): print(v, k)
gram = [i for i, r in enumerate(rows) if "fill" in r["Kernel_Name"] and "rocclr" not in r["Kernel_Name"]]
print("gram fills:", len(gram), [rows[i]["Kernel_Name"][:40] for i in gram[:1]], "durations us", ["%.0f" % ((E(rows[i]) - S(rows[i])) / 1e3) for i in gram])
step = rows[gram[-1]:]
bulk = [r for r in step if isbulk(r)]
t0, t1 = S(step[0]), max(E(r) for r in step)
lastfac = max(E(r) for r in step if "potrf128" in r["Kernel_Name"] or "gemm_nt" in r["Kernel_Name"])
print("step %.2f ms; %d bulk launches, %.2f ms inside" % ((t1 - t0) / 1e6, len(bulk), sum(E(r) - S(r) for r in bulk) / 1e6))
print("before first bulk %.2f ms" % ((S(bulk[0]) - t0) / 1e6))
def seg(bs, label, nxt=None):
    inside = sum(E(r) - S(r) for r in bs) / 1e6
    gaps = sum(max(0, S(bs[i + 1]) - E(bs[i])) for i in range(len(bs) - 1))
    if nxt is not None: gaps += max(0, S(nxt) - E(bs[-1]))
    print("%s: %d launches, inside %.2f ms, gaps %.2f ms, span %.2f ms" % (label, len(bs), inside, gaps / 1e6, ((S(nxt) if nxt is not None else E(bs[-1])) - S(bs[0])) / 1e6))
seg(bulk[:-NT], "before tail", bulk[-NT])
seg(bulk[-NT:], "tail")
print("gaps between bulk launches (us):", " ".join("%.0f" % ((S(bulk[i + 1]) - E(bulk[i])) / 1e3) for i in range(len(bulk) - 1)))
print("after last bulk to last factor kernel %.2f ms; then to end %.2f ms" % ((lastfac - E(bulk[-1])) / 1e6, (t1 - lastfac) / 1e6))
print("--- tail launches (and 4 before): idx queue grid dur_us gap_after_us | block kernels between this launch's start and the next's")
lo = len(bulk) - NT - 4
for i in range(lo, len(bulk)):
    r = bulk[i]
    a = S(r); b = S(bulk[i + 1]) if i + 1 < len(bulk) else lastfac
    pk = [x for x in step if a <= S(x) < b and "potrf128" in x["Kernel_Name"]]
    oth = [x for x in step if a <= S(x) < b and not isbulk(x) and "potrf128" not in x["Kernel_Name"] and "gemm_nt" in x["Kernel_Name"]]
    gap = (S(bulk[i + 1]) - E(r)) / 1e3 if i + 1 < len(bulk) else 0
    print("%2d q%s grid %6d dur %7.1f gap %6.1f | potrf128 %s %s | panel gemms n=%d sum %.0f us" % (
        i, r["Queue_Id"], int(r["Grid_Size_X"]) // 256, (E(r) - S(r)) / 1e3, gap,
        " ".join("%.0f" % ((E(x) - S(x)) / 1e3) for x in pk), "co" if pk and "_co_" in pk[0]["Kernel_Name"] else "8w",
        len(oth), sum(E(x) - S(x) for x in oth) / 1e3))
if len(gram) >= 2:
    i = gram[-1]
    print("--- around the last gram fill")
    for r in rows[max(0, i - 6): i + 3]:
        print("%10.1f %8.1f q%s %s" % ((S(r) - S(rows[i])) / 1e3, (E(r) - S(r)) / 1e3, r["Queue_Id"], r["Kernel_Name"][:70]))
