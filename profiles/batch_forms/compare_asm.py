#!/usr/bin/env python3
"""Compare the device code of mppi_kernels.hip between two commits, function by function.

Inputs: for each side the assembly and the remarks of
  hipcc <the Makefile's FLAGS> -x hip --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
      mppi_kernels.hip -o SIDE.s 2> SIDE.remarks
Usage: compare_asm.py PARENT.s PARENT.remarks NEW.s NEW.remarks

The thirteen batch kernels (finish, claim, ingest) are paired by kernel and form, since their symbol
names changed; every other function is paired by name and must be identical.  Set aside: symbol names,
local label numbers and comments.  Prints the resource table of the thirteen on both sides and, for a
pair whose streams differ, the per-opcode instruction counts that differ and a short unified diff.
Exit status 1 when a pair other than the two tracked ingests differs, or when a tracked ingest differs
in more than kernel-argument load offsets, or when a resource got worse.
"""
import collections
import difflib
import re
import sys

FORMS = ["BatchPlainRun", "BatchIo", "BatchTrackedIo", "BatchCampaign", "BatchScoredCampaign", "BatchWheelRun",
         "BatchWheelCampaign", "BatchWheelScored", "BatchTrack", "BatchWheelTrack"]
BATCH = re.compile(r"mppi_batch_(finish|claim|ingest)_kernel")


def key(sym):
    """(kernel, form) of a batch finish / claim / ingest symbol in either naming, else None."""
    m = BATCH.search(sym)
    if not m:
        return None
    rest = sym[m.end():]
    if rest.startswith("I"):  # a template: the form is its argument (an empty pack: the plain run)
        found = [f for f in FORMS if re.match(r"I(J?)NS_\d+%sE" % f, rest)]
        return (m.group(1), found[0] if found else "BatchPlainRun")
    found = [f for f in FORMS if rest.endswith("%d%sE" % (len(f), f))]  # an overload: its last parameter
    return (m.group(1), found[0] if found else "BatchPlainRun")


def functions(path):
    """name -> the instruction lines of each function of an assembly file."""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not line.startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            out[name] = body
            name = None
        elif s and (not s.startswith(".") or s.startswith(".LBB")):
            body.append(s)
    return out


def normal(body, own):
    """Label numbers in order of first use; the function's own name set aside."""
    seen = {}

    def lab(m):
        return seen.setdefault(m.group(0), ".L%d" % len(seen))

    return [re.sub(r"\.LBB\d+_\d+", lab, l).replace(own, "SELF") for l in body]


def resources(path):
    """name -> {VGPRs, TotalSGPRs, Occupancy, ScratchSize, LDS} from the resource-usage remarks."""
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark: (?:[^:]*: )?\s*(Function Name|VGPRs|TotalSGPRs|Occupancy \[waves/SIMD\]|ScratchSize \[bytes/lane\]"
                      r"|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            out[name] = {}
        elif name:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def opcounts(body):
    return collections.Counter(l.split()[0] for l in body if not l.endswith(":"))


def main():
    pa, pr, na, nr = sys.argv[1:5]
    P, N = functions(pa), functions(na)
    RP, RN = resources(pr), resources(nr)
    pk = {key(n): n for n in P if key(n)}
    nk = {key(n): n for n in N if key(n)}
    bad = 0
    print("| kernel | form | VGPRs p/n | SGPRs p/n | occupancy p/n | scratch p/n | instructions p/n | stream |")
    print("|---|---|---|---|---|---|---|---|")
    details = []
    for k in sorted(pk, key=lambda k: (k[0], FORMS.index(k[1]))):
        if k not in nk:
            print("missing in new:", k)
            bad = 1
            continue
        a, b = normal(P[pk[k]], pk[k]), normal(N[nk[k]], nk[k])
        ra, rb = RP[pk[k]], RN[nk[k]]
        tracked = k[0] == "ingest" and k[1] != "BatchPlainRun"
        if a == b:
            verdict = "identical"
        else:
            ca, cb = opcounts(a), opcounts(b)
            strip = lambda ls: [re.sub(r"(s_load_\w+ .*), 0x[0-9a-f]+$", r"\1, OFF", l) for l in ls]
            if tracked and ca == cb and sorted(strip(a)) != sorted(a):
                verdict = "same opcode counts" + (", differs in kernel-argument offsets only" if strip(a) == strip(b)
                                                  else ", order or registers differ")
            else:
                verdict = "DIFFERS"
                bad = 1
            if ca != cb:
                bad = 1
                details.append("%s %s opcode counts: %s" % (k[0], k[1], {o: (ca[o], cb[o]) for o in set(ca) | set(cb)
                                                                       if ca[o] != cb[o]}))
            details.append("%s %s:\n" % k + "\n".join(list(difflib.unified_diff(a, b, "parent", "new", n=1, lineterm=""))[:60]))
        worse = rb["VGPRs"] > ra["VGPRs"] or rb["Occupancy"] < ra["Occupancy"] or rb["ScratchSize"] > ra["ScratchSize"]
        bad |= worse
        print("| %s | %s | %d/%d | %d/%d | %d/%d | %d/%d | %d/%d | %s%s |" % (
            k[0], k[1], ra["VGPRs"], rb["VGPRs"], ra["TotalSGPRs"], rb["TotalSGPRs"], ra["Occupancy"], rb["Occupancy"],
            ra["ScratchSize"], rb["ScratchSize"], len(a), len(b), verdict, ", RESOURCES WORSE" if worse else ""))
    others_p = {n: b for n, b in P.items() if not key(n)}
    others_n = {n: b for n, b in N.items() if not key(n)}
    diff = [n for n in sorted(set(others_p) | set(others_n))
            if n not in others_p or n not in others_n or normal(others_p[n], n) != normal(others_n[n], n)]
    print("\nother functions: %d in the parent, %d in the new file, %d differ or are missing%s" % (
        len(others_p), len(others_n), len(diff), (": " + ", ".join(diff)) if diff else ""))
    bad |= bool(diff)
    for d in details:
        print("\n" + d)
    return int(bad)


if __name__ == "__main__":
    sys.exit(main())
