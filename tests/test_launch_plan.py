"""The launch planner (csrc/gm_plan.cpp): how the HMC/MH and NUTS drivers cut
a run into kernel launches. Host-only integer arithmetic, so it is built with
the host compiler under AddressSanitizer + UBSan together with
tools/plan_dump.cpp and run directly, without a GPU.

Checked: the plans recorded from the three HMC loops and the NUTS segment
block that the planner replaced (tests/golden/launch_plans.json), and the
conditions a plan must meet whatever produced it, on those cases and on random
small parameters: the slab cap of the pooled metric and NUTS's trailing
re-find segment, which no GPU test reaches within seconds, among them."""
import json
import os
import random
import shutil
import subprocess

import pytest

from tests import _hmc_adapt_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++"
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.json")

pytestmark = pytest.mark.skipif(not shutil.which(CXX), reason="needs the ROCm toolchain's clang++")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_dump")
    r = subprocess.run([CXX, "-std=c++20", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "plan_dump.cpp"),
                        os.path.join(ROOT, "general-mcmc_amd", "csrc", "gm_plan.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    def run(lines):
        """One plan per input line: (segments [start, n, cf, row0, warm, update, first_used, used], end state)."""
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
        p = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                           timeout=120, env=env)
        assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-3000:]
        plans, segs = [], []
        for l in p.stdout.splitlines():
            t = l.split()
            if t[0] == "seg":
                segs.append([int(x) for x in t[1:]])
            else:
                assert t[0] == "end"
                assert int(t[3]) == len(segs)
                plans.append((segs, [int(t[1]), int(t[2])]))
                segs = []
        assert len(plans) == len(lines)
        return plans
    return run


def hmc_line(c):
    return "hmc {variant} {total} {chunk} {collect_from} {warm} {sb} {eb} {iw} {slab_rows}".format(**c)


def nuts_line(c, r):
    return "nuts {total} {chunk} {n_discard} {windows} {sb} {eb} {s0} {s1} {slab_rows}".format(
        sb=c["sb"], eb=c["eb"], s0=r["sched_in"][0], s1=r["sched_in"][1], **r)


def fresh_schedule(sb, iw):
    return [max(sb, 1) + max(iw, 10), max(iw, 10)]


def check_plan(segs, *, total, chunk, warm, cut_at_warm, ends, sb, lim, slab_rows, nuts, what):
    """The conditions on a plan (segments as run() returns them). ends: the
    window ends by tests/_hmc_adapt_ref.window_ends, None where that schedule
    does not apply (a NUTS run that continues an earlier run's schedule)."""
    # 1. the segments tile [0, total) in order
    pos = 0
    for i, (start, n, _cf, _row0, _w, upd, _first, _used) in enumerate(segs):
        assert start == pos, what
        trailing = nuts and n == 0 and i == len(segs) - 1 and (total <= 0 or (i > 0 and segs[i - 1][5]))
        assert (1 <= n <= chunk) or trailing, (what, i, n)
        pos += n
    assert pos == max(total, 0), what
    if nuts:
        assert len(segs) >= 1, what
        # an update on the run's last transition is followed by the re-find segment
        upd_last = [i for i, s in enumerate(segs) if s[5] and s[0] + s[1] == total]
        assert all(i + 1 < len(segs) and segs[i + 1][1] == 0 for i in upd_last), what
    else:
        assert all(s[1] >= 1 for s in segs), what
    # 2. no segment straddles the warm-up's end
    if cut_at_warm:
        assert all(not (s[0] < warm < s[0] + s[1]) for s in segs), what
    # 3. the updates are the window ends
    if ends is not None:
        assert [s[0] + s[1] for s in segs if s[5]] == [m for m in ends if m <= total], what
    # 4. window rows
    rows = []
    for start, n, _cf, _row0, _w, _upd, first, used in segs:
        if used:
            assert start < first and first + used - 1 <= start + n, what
            rows += range(first, first + used)
            if slab_rows:
                assert used <= slab_rows and start + n <= lim - 1, what
    if slab_rows:
        assert rows == [m for m in range(1, total + 1) if sb < m < lim], what
    # 5. a segment is as long as the cuts allow
    for start, n, _cf, _row0, _w, upd, _first, used in segs:
        end = start + n
        if n < chunk and not (nuts and n == 0):
            assert (end == total or (cut_at_warm and end == warm) or upd or
                    (slab_rows and (used == slab_rows or end == lim - 1))), (what, start, n)


def test_golden_plans(dump):
    """The planner gives the launches of the loops it replaced, case by case."""
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 45
    lines, keys = [], []
    for c in cases:
        if c["sampler"] == "hmc":
            lines.append(hmc_line(c))
            keys.append((c, None))
        else:
            for r in c["runs"]:
                lines.append(nuts_line(c, r))
                keys.append((c, r))
    for (c, r), (segs, end) in zip(keys, dump(lines)):
        if r is None:
            # (start, n, cf, row0, warm-up?, update, used)
            assert [[s[0], s[1], s[2], s[3], s[4], s[5], s[7]] for s in segs] == c["launches"], c["name"]
            windows = c["variant"] in ("adapt2", "dense")
            lim = max(c["warm"] - c["eb"], 0)
            check_plan(segs, total=c["total"], chunk=c["chunk"], warm=c["warm"], cut_at_warm=True,
                       ends=ref.window_ends(c["warm"], c["sb"], c["eb"], c["iw"]) if windows else [],
                       sb=c["sb"], lim=lim, slab_rows=c["slab_rows"], nuts=False, what=c["name"])
        else:
            # (start, n, update, first_used, used)
            assert [[s[0], s[1], s[5], s[6], s[7]] for s in segs] == r["launches"], c["name"]
            assert end == r["sched_out"], c["name"]
            ends = None
            if not r["windows"]:
                ends = []
            elif r["sched_in"] == fresh_schedule(c["sb"], c["iw"]):
                ends = ref.window_ends(r["n_discard"], c["sb"], c["eb"], c["iw"])
            check_plan(segs, total=r["total"], chunk=r["chunk"], warm=0, cut_at_warm=False, ends=ends, sb=c["sb"],
                       lim=max(r["n_discard"] - c["eb"], 0), slab_rows=r["slab_rows"], nuts=True, what=c["name"])


def test_golden_cases_named_by_the_schedule():
    """The recorded cases hold what they were chosen for."""
    with open(GOLDEN) as f:
        cases = {c["name"]: c for c in json.load(f)["cases"]}
    assert ref.window_ends(60, 5, 10, 10) == [15, 25, 45, 49]
    for name in ("adapt2-w60-c20-k7", "adapt2-w60-c20-k1000", "dense-s3-w60-c20-k7"):
        assert [s[0] + s[1] for s in cases[name]["launches"] if s[5]] == [15, 25, 45, 49], name
    assert not any(s[5] for s in cases["adapt2-w60-c20-k7-noends"]["launches"])
    assert cases["plain-0-4"]["launches"] == []
    assert cases["nuts-total0"]["runs"][0]["launches"] == [[0, 0, 0, 0, 0]]
    for name in ("nuts-end-on-last", "nuts-pooled-end-on-last"):
        last, refind = cases[name]["runs"][0]["launches"][-2:]
        assert last[0] + last[1] == 49 and last[2] == 1 and refind == [49, 0, 0, 0, 0], name
    two = cases["nuts-two-runs"]["runs"]
    assert two[1]["sched_in"] == two[0]["sched_out"] != two[0]["sched_in"]


def test_random_plans(dump):
    """The conditions on a few hundred random small parameter sets."""
    rng = random.Random(20240611)
    lines, checks = [], []
    for i in range(400):
        total, chunk = rng.randint(0, 120), rng.choice([1, 2, 3, 5, 7, 16, 40, 1000])
        sb, eb, iw = rng.randint(0, 20), rng.randint(0, 20), rng.randint(0, 30)
        slab = rng.choice([1, 2, 3, 5, 10**6])
        if i % 2 == 0:
            variant = rng.choice(["plain", "adapt1", "adapt2", "dense"])
            warm = 0 if variant == "plain" else rng.randint(0, total)
            c = dict(variant=variant, total=total, chunk=chunk, collect_from=rng.randint(0, total), warm=warm, sb=sb,
                     eb=eb, iw=iw, slab_rows=slab if variant == "dense" else 0)
            lines.append(hmc_line(c))
            windows = variant in ("adapt2", "dense")
            checks.append(dict(total=total, chunk=chunk, warm=warm, cut_at_warm=True,
                               ends=ref.window_ends(warm, sb, eb, iw) if windows else [], sb=sb,
                               lim=max(warm - eb, 0), slab_rows=c["slab_rows"], nuts=False, what=lines[-1]))
        else:
            nd, windows = rng.randint(0, 100), rng.randint(0, 1)
            r = dict(total=total, chunk=chunk, n_discard=nd, windows=windows, sched_in=fresh_schedule(sb, iw),
                     slab_rows=slab if windows and rng.randint(0, 1) else 0)
            lines.append(nuts_line(dict(sb=sb, eb=eb), r))
            checks.append(dict(total=total, chunk=chunk, warm=0, cut_at_warm=False,
                               ends=ref.window_ends(nd, sb, eb, iw) if windows else [], sb=sb, lim=max(nd - eb, 0),
                               slab_rows=r["slab_rows"], nuts=True, what=lines[-1]))
    for (segs, _end), kw in zip(dump(lines), checks):
        check_plan(segs, **kw)
        if not kw["nuts"]:  # the collection window of every HMC launch stays inside it
            assert all(0 <= s[2] <= s[1] and s[3] >= 0 for s in segs), kw["what"]
