"""The native HOST code (csrc/host_db.cpp, host_group.cpp, host_refine.cpp, host_stage.cpp, np_dispatch.h; tuning.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer.  Every other test of that code compares VALUES; a read
one element past a label row, a write one record past a pool's capacity, a signed overflow or an unsynchronised static give the
right values and are still bugs.  Sanitizers are off limits on the device, so the host build is where they go: a host-only
replay harness (tests/native/host_replay.cpp; no Python, no HIP; `make -C comic-text-detector_amd/csrc san OUT=<dir>`) replays
calls recorded from the shipped library (tests/host_replay.py) with every buffer an exact-size heap allocation of its own,
serially and on 8 threads.  CPU only; nothing here touches a GPU or sets anything about how Python starts."""
import math
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import host_replay as HR
from conftest import ROOT, pkg
from sweep_cases import equal_up_to_tied_lines

CSRC = os.path.join(ROOT, "comic-text-detector_amd", "csrc")
SAN_FLAG = {"plain": "", "asan": "-fsanitize=address,undefined,float-cast-overflow", "tsan": "-fsanitize=thread"}
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1", "TSAN_OPTIONS": "halt_on_error=1"}
THREADS = 8
ERR_NOMEM = HR.ERR_NOMEM


def _run(cmd, timeout):
    env = dict(os.environ, **SAN_ENV)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("host_san"))


@pytest.fixture(scope="module")
def flavours(work):
    """{flavour: None if usable, else the reason to skip}: a flavour is skipped only when a one-line program fails to link
    with its -fsanitize flag (the compiler's message), or links and cannot start on this host (the runtime's message)."""
    src = os.path.join(work, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    out = {}
    for fl, flag in SAN_FLAG.items():
        exe = os.path.join(work, "probe_" + fl)
        r = subprocess.run(["g++", *flag.split(), src, "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            out[fl] = f"g++ {flag} does not link here: {(r.stderr or r.stdout).strip()[-300:]}"
            continue
        r = _run([exe], 60)
        out[fl] = None if r.returncode == 0 else f"a program built with {flag} does not start here: {(r.stderr or r.stdout).strip()[-300:]}"
    assert out["plain"] is None, out["plain"]
    return out


@pytest.fixture(scope="module")
def built(work, flavours):
    """`make san` for the usable flavours into the test's own directory; the shipped library and its build stay untouched."""
    lib = pkg()._lib.LIB_PATH
    before = os.stat(lib).st_mtime_ns if os.path.exists(lib) else None
    use = [fl for fl, why in flavours.items() if why is None]
    r = subprocess.run(["make", "-C", CSRC, "-j4", "san", "OUT=" + work, "SAN_FLAVOURS=" + " ".join(use)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "hipcc" not in r.stdout and "/opt/rocm" not in r.stdout, "the san target must not need ROCm"
    assert before == (os.stat(lib).st_mtime_ns if os.path.exists(lib) else None), "make san touched libctd_hip.so"
    return {fl: os.path.join(work, "host_replay_" + fl) for fl in use}


@pytest.fixture(scope="module")
def case_set(work):
    rec = HR.build_case_set()
    path = os.path.join(work, "cases.bin")
    HR.write_cases(path, rec.cases)
    return rec.cases, path


_RESULTS = {}


def replay(built, flavours, case_set, work, flavour, mode):
    """(exit status, stdout, stderr, results) of one harness run; each child under a timeout of its own."""
    if flavours[flavour] is not None:
        pytest.skip(flavours[flavour])
    key = (flavour, mode)
    if key not in _RESULTS:
        out = os.path.join(work, f"results_{flavour}_{mode}.bin")
        r = _run([built[flavour], case_set[1], out] + (["serial"] if mode == "serial" else ["threads", str(THREADS)]), 600)
        _RESULTS[key] = (r.returncode, r.stdout, r.stderr, HR.read_results(out) if r.returncode == 0 else [])
    return _RESULTS[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------- 1. plain harness == shipped library

def libm_distance(c, d):
    """`abs(math.sin(math.acos(c)) * d)`: Python's math is the harness's libm."""
    if not (-1.0 <= c <= 1.0):
        return math.nan                          # numpy's / libm's arccos outside its domain (and of a nan)
    return abs(math.sin(math.acos(c)) * d)


def _blocks(res, TB):
    nb, nl, nd = (int(res[k][0]) for k in ("n_blk_out", "n_lines_out", "n_dist_out"))
    recs = np.frombuffer(res["blks"].tobytes(), TB.BLK_DTYPE)[:nb]
    return recs, res["lines_out"].reshape(-1, 8)[:nl], res["dist_out"].reshape(-1, 3)[:nd]


def compare_group(case, res, TB):
    """'' if the harness's `ctd_group_output` equals the recorded call in everything but the one library-dependent value (the
    first member of every distance triple, checked against libm exactly: its operands c and d are compared bit for bit),
    'tie...' if the only further difference is the order of lines whose distances tie (or a split that order decided: the
    page's lines are the same multiset), else what differs."""
    exp = case["expected"]
    if int(res["rc"][0]) != int(exp["rc"][0]):
        return f"rc {int(res['rc'][0])} != {int(exp['rc'][0])}"
    if int(exp["rc"][0]) != 0:
        return ""
    grecs, glines, gdist = _blocks(res, TB)
    erecs, elines, edist = _blocks(exp, TB)
    for i, (c, d, v) in enumerate(zip(gdist[:, 1].tolist(), gdist[:, 2].tolist(), gdist[:, 0].tolist())):
        want = libm_distance(c, d)
        if not (v == want or (v != v and want != want)):
            return f"distance {i}: {v!r} is not abs(sin(acos({c!r})) * {d!r}) = {want!r}"
    fields = [n for n in TB.BLK_DTYPE.names if n != "pad_"]
    exact = (len(grecs) == len(erecs) and all(same_bits(grecs[n], erecs[n]) for n in fields) and same_bits(glines, elines)
             and same_bits(gdist[:, 1:], edist[:, 1:]))
    if exact:
        return ""
    # what a tie cannot change: the return code (above), the number of lines, the page's lines as a multiset
    if len(glines) != len(elines) or sorted(map(tuple, glines.tolist())) != sorted(map(tuple, elines.tolist())):
        return "the pages' lines differ as multisets"
    got, ref = TB.blocks_from_records(grecs, glines, gdist), TB.blocks_from_records(erecs, elines, edist)
    return "tie" if equal_up_to_tied_lines(got, ref) else "tie, and the order decided a split"


def compare_topk(case, res):
    """'' / 'tie' / what differs: bins of EQUAL count may be picked in another order (numpy's argsort against a stable sort);
    everything before the first such pick must agree, what follows it may not be compared."""
    exp = case["expected"]
    if same_bits(res["rc"], exp["rc"]) and same_bits(res["colors"], exp["colors"]):
        return ""
    hist = case["items"]["hist"]
    px = np.repeat(np.arange(256, dtype=np.uint8), hist)
    counts, edges = np.histogram(px, bins=255)
    count_of = {float(e): int(c) for e, c in zip(edges[:-1], counts)}
    for k in range(min(int(res["rc"][0]), int(exp["rc"][0]))):
        a, b = float(res["colors"][k]), float(exp["colors"][k])
        if a != b:
            return "tie" if a in count_of and b in count_of and count_of[a] == count_of[b] else f"colour {k}: {a} != {b}"
    return "tie" if count_of and Counter(count_of.values()).most_common(1)[0][1] > 1 else "the colour counts differ"


def test_plain_harness_equals_the_shipped_library(built, flavours, case_set, work):
    """What ties the harness to the code the product runs: the -O2 harness against the results the shipped library gave in
    this process.  The harness holds no numpy, so csrc/np_dispatch.h takes its libm / stable-sort side there while the recording
    took numpy's; the distance value and the order of TIES may differ, on the generators that construct ties only."""
    TB = pkg().textblock
    cases, _ = case_set
    rc, out, err, results = replay(built, flavours, case_set, work, "plain", "serial")
    assert rc == 0 and err == "", (rc, out[-2000:], err[-2000:])
    assert [r[0] for r in results] == [c["name"] for c in cases]
    per_entry = Counter(c["entry"] for c in cases)
    print("\ncases per entry point:", dict(per_entry))
    assert set(per_entry) == {"ctd_group_output", "ctd_db_boxes", "ctd_db_boxes_compact", "ctd_topk_colors", "ctd_otsu_from_hist",
                              "ctd_inrange_bounds", "refine_rules", "refine_candidates", "ctd_host_gather"}
    bad, ties = [], Counter()
    by_name = {}
    for case, (name, entry, res) in zip(cases, results):
        by_name[name] = res
        if entry == "ctd_group_output":
            verdict = compare_group(case, res, TB)
        elif entry == "ctd_topk_colors":
            verdict = compare_topk(case, res)
            # ... and whatever the ties do: the harness is the reference's code where numpy has libm and a stable sort
            want = HR.topk_by_the_oracle(case["py"], libm_side=True)
            if res["colors"][: int(res["rc"][0])].tolist() != want:
                verdict = f"colours {res['colors'].tolist()} are not the oracle's with a stable sort {want}"
        else:
            verdict = ""                                     # bit for bit (the tied xor sums of `refine_candidates` carry no values)
            for tag, want in case["expected"].items():
                got = res[tag].reshape(-1)[: want.size] if tag not in ("rc", "n_out") else res[tag]
                if not same_bits(got, want.reshape(-1)):
                    verdict = f"{tag} differs"
                    break
        if verdict.startswith("tie"):
            ties[(entry, verdict, "constructed ties" if case["tied"] else "no constructed ties")] += 1
            if not case["tied"]:
                bad.append((name, "differs by a tie although its generator constructs none"))
        elif verdict:
            bad.append((name, verdict))
    print("tie-only differences (entry point, generator constructs ties):", dict(ties))
    assert not bad, (len(bad), bad[:10])
    # the documented failure side, case by case, in the shipped library's record AND in the harness: a pool one below what the
    # page needs is CTD_ERR_NOMEM, exactly the need is enough and gives those counts; a candidate cap below the contour count
    # truncates to the cap (the recorder states each case's intent when it builds it)
    n_intent = Counter()
    for c in cases:
        intent = c.get("intent")
        if intent is None:
            continue
        for who, got in (("record", c["expected"]), ("harness", by_name[c["name"]])):
            assert int(got["rc"][0]) == intent["rc"], (c["name"], who, int(got["rc"][0]), intent)
            if "counts" in intent:
                assert [int(got[k][0]) for k in ("n_blk_out", "n_lines_out", "n_dist_out")] == intent["counts"], (c["name"], who)
            if "n_out" in intent:
                assert int(got["n_out"][0]) == intent["n_out"], (c["name"], who, int(got["n_out"][0]), intent)
        kind = "nomem" if intent["rc"] == ERR_NOMEM else "exact" if "counts" in intent else \
            "truncated" if intent["n_out"] < intent["contours"] else "all contours"
        n_intent[(c["entry"], kind)] += 1
    print("cases with a stated outcome:", dict(n_intent))
    assert n_intent[("ctd_group_output", "nomem")] >= 12 and n_intent[("ctd_group_output", "exact")] >= 6
    assert n_intent[("ctd_db_boxes", "truncated")] >= 20 and n_intent[("ctd_db_boxes_compact", "truncated")] >= 20
    # a mask whose pitch exceeds its width changes nothing
    for c in cases:
        if "same_as" in c:
            a, b = by_name[c["name"]], by_name[c["same_as"]]
            assert all(same_bits(a[k][: a[k].size], b[k].reshape(-1)[: a[k].size]) for k in ("lines_out", "dist_out", "blks"))


# ------------------------------------------------------------------------------- the condition on the tie-free generators

def test_tie_free_pages_tie_nowhere_by_the_oracle_alone(case_set):
    """The cap of 0 tie-only differences on the page generators without constructed ties is a CONDITION: from the oracle alone
    (no product code), the oracle with libm's acos and a stable sort must give what the oracle with numpy's own gives -- the
    same blocks with the same lines in the same order.  The 300 random histograms are NOT held to that cap, a deviation from
    what was asked: the empty bins of a sparse histogram tie, 52 of the 300 pick a colour among them, and tests/host_replay.py
    files exactly those under the tie cases by this comparison (so asserting it on the rest would prove nothing).  Every
    histogram's colours and rules, tied or not, must equal the oracle's with a stable sort in the test above."""
    import copy
    from oracle import postproc_ref as R
    cases, _ = case_set
    n_pages, broken = 0, []
    for c in cases:
        if c["tied"] or "py" not in c or c["entry"] != "ctd_group_output":
            continue
        blks, lines, im_w, im_h, mask = c["py"]
        lines = np.asarray(lines, np.int32).reshape(-1, 4, 2)
        with np.errstate(all="ignore"):
            a = R.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask)
            with HR.numpy_on_the_libm_side():
                b = R.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask)
        same = len(a) == len(b) and all(list(x.xyxy) == list(y.xyxy) and np.array_equal(np.asarray(x.lines), np.asarray(y.lines))
                                        and (x.vertical, x.angle, x.font_size) == (y.vertical, y.angle, y.font_size)
                                        for x, y in zip(a, b))
        n_pages += 1
        if not same:
            broken.append(c["name"])
    print(f"\noracle alone, numpy's arccos / argsort against libm / stable: {n_pages} pages, differing: {broken}")
    assert n_pages >= 25
    assert not broken, broken


# --------------------------------------------------------------------------------------------------- 2. under the sanitizers

@pytest.mark.parametrize("flavour,mode", [("plain", "threads"), ("asan", "serial"), ("asan", "threads"), ("tsan", "serial"),
                                          ("tsan", "threads")])
def test_sanitized_harness_is_silent_and_equals_the_plain_one(built, flavours, case_set, work, flavour, mode):
    """Exit status 0, nothing on stderr (a sanitizer report goes there), no exception, and every output buffer of every case
    bit for bit what the plain harness wrote serially -- in `threads` mode for both copies of every case."""
    _, _, _, plain = replay(built, flavours, case_set, work, "plain", "serial")
    rc, out, err, results = replay(built, flavours, case_set, work, flavour, mode)
    assert rc == 0 and err == "", f"{flavour} {mode}: exit status {rc}\n{out[-1500:]}\n{err[-6000:]}"
    assert "0 exceptions" in out
    copies = 2 if mode == "threads" else 1
    assert len(results) == copies * len(plain)
    bad = []
    for i, (name, entry, res) in enumerate(results):
        pname, pentry, pres = plain[i // copies]
        if name != (pname + f"#{i % copies}" if copies == 2 else pname) or entry != pentry or list(res) != list(pres) or \
           not all(same_bits(res[k], pres[k]) for k in res):
            bad.append(name)
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------------------- 3. the canary

@pytest.mark.parametrize("flavour,defect,report", [("asan", "heap", "heap-buffer-overflow"), ("asan", "overflow", "signed integer overflow"),
                                                   ("tsan", "race", "data race")])
def test_canary_is_reported(built, flavours, work, flavour, defect, report):
    """A -fsanitize flag dropped from the `san` rule must not turn this file green: the same rule builds three deliberate
    defects (tests/native/san_canary.cpp), and each sanitizer must REPORT its own."""
    if flavours[flavour] is not None:
        pytest.skip(flavours[flavour])
    r = _run([os.path.join(work, "san_canary_" + flavour), defect], 120)
    assert r.returncode != 0 and report in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.mark.parametrize("defect", ["heap", "overflow", "race"])
def test_canary_is_silent_in_the_plain_flavour(built, work, defect):
    r = _run([os.path.join(work, "san_canary_plain"), defect], 120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])


# ------------------------------------------------------------------------------------------------------ 4. the tuning table

# The ONE place outside csrc/tuning.def that knows a default: key -> (type, default, lower bound or None, engines re-plan),
# transcribed from the sources as they were before the table existed.  Retuning a default is an edit of its row there and here.
TUNING_PIN = {
    "fuse": ("int", 63, None, True), "c3_min_patches": ("long long", 1024, None, True),
    "c3b_min_patches": ("long long", 1024, None, True), "c3b_max_ch": ("int", 128, None, True),
    "c3b_cfg64": ("int", 0, None, True), "c3b_cfg128": ("int", 1, None, True),
    "seg_final_mfma": ("int", 1, None, True), "db_up_mfma": ("int", 1, None, True),
    "halo": ("int", 1, None, True), "halo_min_patches": ("long long", 1024, None, True), "halo_pair": ("int", 1, None, True),
    "halo3": ("long long", 1, None, True), "halo3_min_blocks": ("long long", 1024, None, True),
    "no_reuse": ("int", 0, None, True), "f32_mfma": ("int", 1, None, True), "fwd_prio": ("int", 1, None, True),
    "split_stem": ("int", 1, None, True), "split_planes": ("int", 1, None, True), "split_halo": ("int", 1, None, True),
    "split_halo_min_patches": ("long long", 512, None, True),
    "tail_max_blocks": ("int", 1024, 1, False), "tail_chain": ("int", 1, None, False),
    "tail_lds": ("int", 1, None, False), "tail_lds_rcap": ("int", 0, None, False),
    "tail_lds_max_bytes": ("long long", 150 << 10, None, False), "tail_lds_runs_x10": ("int", 25, 1, False),
    "tail_lds_threads": ("int", 512, None, False), "tail_lds_cls0": ("long long", 40 << 10, None, False),
    "tail_lds_cls1": ("long long", 80 << 10, None, False), "tail_dma_min": ("long long", 256 << 10, None, False),
    "tail_priority": ("int", 1, None, False), "tail_cus": ("int", 0, None, False), "tail_cu_first": ("int", 0, None, False),
}


def test_tuning_table_holds_the_pinned_defaults_with_and_without_the_sanitizers(flavours, work):
    """tests/native/tuning_table.cpp (tuning.cpp alone, its own main): every row's type, default, replan flag, what it stores
    for a value below any lower bound (-7) and for 1 << 40 (an int key keeps the low 32 bits, a long long key all of it),
    unknown keys and null pointers refused with nothing written, every key restored.  The -O2 build and the ASan + UBSan build
    print the same, the sanitized one nothing else, and both print TUNING_PIN."""
    if flavours["asan"] is not None:
        pytest.skip(flavours["asan"])
    r = subprocess.run(["make", "-C", CSRC, "-j2", "san_tuning", "OUT=" + work, "SAN_FLAVOURS=plain asan"], capture_output=True, text=True)
    assert r.returncode == 0 and "hipcc" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    runs = {fl: _run([os.path.join(work, "tuning_table_" + fl)], 120) for fl in ("plain", "asan")}
    for fl, r in runs.items():
        assert r.returncode == 0 and r.stderr == "", (fl, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert runs["plain"].stdout == runs["asan"].stdout
    assert len(TUNING_PIN) == 33
    assert all(replan == (not key.startswith("tail_")) for key, (_, _, _, replan) in TUNING_PIN.items())
    want = sorted(f"{key} {typ} {default} {int(replan)} {-7 if low is None else low} {0 if typ == 'int' else 1 << 40}"
                  for key, (typ, default, low, replan) in TUNING_PIN.items())
    *rows, unknown, restored = runs["plain"].stdout.splitlines()
    assert sorted(rows) == want and len(rows) == len(set(rows))
    assert unknown == "unknown key: set -1 get -1, null key: set -1 get -1, null value: get -1, untouched 12345 0"
    assert restored == "restored 33 keys"
