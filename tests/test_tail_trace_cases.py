"""The cases of tests/test_gpu_tail_trace.py (tests/tail_trace_cases.py) checked WITHOUT a GPU, from the oracle alone: the
windows the generator's blocks produce cover every shape class the window kernels treat differently (nothing can go vacuous
after an edit of the generator), the pages are adversarial where a wrong kernel would read, the references satisfy what the
GPU test requires of the device, and every compare helper reports a result that is the reference with ONE element perturbed."""
import functools

import numpy as np
import pytest

import tail_trace_cases as T


@functools.lru_cache(None)
def _wc():
    case = T.width_class_case()
    return case, T.refine_reference(case)


def _windows(case):
    return [(b, w) for b, (img, boxes) in enumerate(zip(case["pages"], case["boxes"])) for w in T.windows_of(img.shape, boxes)]


# ---------------------------------------------------------------------------------------------------------- refine: coverage

def test_width_class_page_covers_every_shape_class():
    case, _ = _wc()
    assert [p.shape[1] for p in case["pages"]] == [203, 201, 202, 200]           # widths that are no multiple of 4 among them
    for b, (img, boxes) in enumerate(zip(case["pages"], case["boxes"])):
        im_h, im_w = img.shape[:2]
        wins = T.windows_of(img.shape, boxes)
        assert wins == T.width_class_windows(im_w, im_h)                         # the blocks give exactly the intended windows
        sizes = {(w, h) for _, _, w, h in wins}
        for w in T.WIDTHS:
            for h in (1, 2, 3):
                assert (w, h) in sizes, (w, h)
            assert any(ww == w and hh >= 8 for ww, hh in sizes), w
        assert {w % 4 for _, _, w, _ in wins if w < 8} == {0, 1, 2, 3} == {w % 4 for _, _, w, _ in wins if w >= 8}
        assert {x % 4 for x, _, w, _ in wins if w < 8} == {0, 1, 2, 3} == {x % 4 for x, _, w, _ in wins if w >= 8}
        left, top = {i for i, w in enumerate(wins) if w[0] == 0}, {i for i, w in enumerate(wins) if w[1] == 0}
        right = {i for i, w in enumerate(wins) if w[0] + w[2] == im_w - 1}       # the reference clamps at im_w - 1
        bottom = {i for i, w in enumerate(wins) if w[1] + w[3] == im_h - 1}
        assert left and top and right and bottom
        assert left & top and right & top and left & bottom and right & bottom   # the four corners


def test_pages_are_adversarial_outside_their_windows():
    """A kernel that counted pixels beyond the window as 0, read the page's mask beyond it, took >= 127 for > 127 or left
    out the last column must change the grey histogram on MANY windows of each instantiation (w < 8 and w >= 8), not on a few
    per cent (measured: see the floors)."""
    case, (recs, _, _) = _wc()
    hits = {k: {False: 0, True: 0} for k in ("page0", "page", "ge127", "lastcol")}
    total = {False: 0, True: 0}
    for rec, (b, win) in zip(recs, _windows(case)):
        x1, y1, w, h = win
        img, msk = case["pages"][b], case["masks"][b]
        crop_i, crop_m = img[y1: y1 + h, x1: x1 + w], msk[y1: y1 + h, x1: x1 + w]
        assert np.array_equal(T.hist_with(crop_i, crop_m, "right"), rec["hist"][0])
        fast = w >= 8
        total[fast] += 1
        for k in ("page0", "ge127", "lastcol"):
            hits[k][fast] += not np.array_equal(T.hist_with(crop_i, crop_m, k), rec["hist"][0])
        hits["page"][fast] += not np.array_equal(T.hist_reading_the_page(img, msk, win), rec["hist"][0])
    print("\nwindows whose grey histogram a wrong kernel changes (w < 8, w >= 8):", hits, "of", total)
    for k, floor in (("page0", 0.3), ("page", 0.3), ("ge127", 0.25), ("lastcol", 0.25)):
        for fast in (False, True):
            assert hits[k][fast] >= floor * total[fast], (k, fast, hits[k], total)


def test_image_kinds():
    case, _ = _wc()
    for b, kind in enumerate(T.IMAGE_KINDS):
        img = case["pages"][b]
        wins = T.windows_of(img.shape, case["boxes"][b])
        # waves of the histogram kernel: 64 groups of 4 pixels along the window; distinct greys per window is what matters here
        colours = [len(np.unique(img[y: y + h, x: x + w].reshape(-1, 3), axis=0)) for x, y, w, h in wins if w * h >= 16]
        if kind == "flat":
            assert max(colours) == 1                      # one bin per wave: the first arm of hist_add only
        elif kind == "two-valued":
            assert max(colours) == 2 and min(colours) >= 1
        elif kind == "noisy":
            assert min(colours) > 2                       # more than two bins per wave: all three arms
        covered = np.zeros(img.shape[:2], bool)
        for x, y, w, h in wins:
            covered[y: y + h, x: x + w] = True
        if kind == "grey":                                # B = G = R inside every window: the three Otsu channels tie
            assert np.array_equal(img[covered][:, 0], img[covered][:, 1]) and np.array_equal(img[covered][:, 0], img[covered][:, 2])
            assert min(colours) > 2
        assert len(np.unique(img[~covered].reshape(-1, 3), axis=0)) > 1000      # random colours outside, whatever the kind


def test_big_windows_and_calls():
    cases = {c["name"]: c for c in T.refine_cases()}
    assert len(cases) == 6
    by = lambda frag: next(c for n, c in cases.items() if frag in n)                                    # noqa: E731
    w2 = _windows(by("96 x 48 alone"))
    assert len(w2) == 1 and 4096 < w2[0][1][2] * w2[0][1][3] <= 8192            # two blocks of 4 096 pixels
    w4 = _windows(by("131 x 97 alone"))
    px = w4[0][1][2] * w4[0][1][3]
    assert len(w4) == 1 and px >= 12000 and (px + 4095) // 4096 == 4 and w4[0][1][2] % 4 != 0
    groups = (w4[0][1][2] + 3) // 4 * w4[0][1][3]
    assert groups > 2 * 4 * 256                                                    # several grid-stride trips of 4 blocks x 256
    mixed = [w for _, w in _windows(by("big, tiny"))]
    assert T.BIG2 in mixed and T.BIG4 in mixed and (7, 5, 1, 1) in mixed and (13, 9, 3, 2) in mixed
    assert len(mixed) != len(set(mixed))                                           # the same window twice
    overlap = lambda a, b: a != b and a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]  # noqa: E731
    assert any(overlap(a, b) for a in mixed for b in mixed)
    capped = by("tail_max_blocks")
    low, = capped["tune"].values()
    assert 1 <= low // len(_windows(capped)) < 4                                   # fewer blocks per window than the largest asks for
    three = by("three pages")
    assert len({p.shape[1] for p in three["pages"]}) == 3 and all(len(b) >= 5 for b in three["boxes"])
    keep = by("keep_undetected_mask")
    recs, refined, after = T.refine_reference(keep)
    assert keep["keep"] and sum(r["pass_"] == 1 for r in recs) >= 3 and sum(r["pass_"] == 0 for r in recs) == 2
    assert [r["pass_"] for r in recs] == sorted(r["pass_"] for r in recs)         # pass 0 first
    assert not np.array_equal(after[0], keep["masks"][0])                         # refine_undetected_mask edited the mask


def test_references_satisfy_what_the_gpu_test_requires():
    _, (recs, refined, _) = _wc()
    assert len(recs) == 4 * len(T.width_class_windows())
    nonempty = 0
    for r in recs:
        assert 1 <= r["n_cand"] <= 4 and r["hist"].shape == (4, 256) and r["rules"].shape == (6, 3)
        assert (r["hist"][1:].sum(axis=1) == r["w"] * r["h"]).all() and r["hist"][0].sum() <= r["w"] * r["h"]
        assert not r["sums"][r["rules"][:, 0] < 0].any()                          # an unused rule's sum is 0
        assert (r["sums"] <= 255 * r["w"] * r["h"]).all()
        assert list(r["cand_dist"]) == sorted(r["cand_dist"])
        nonempty += bool(r["hist"][0].any())
        T.compare_window(T.as_record(r), r)
    assert nonempty >= len(recs) // 3                                             # eroded selections exist (levels 127 / 128 decide)
    assert all(m.any() for m in refined)


# ------------------------------------------------------------------------------------------ refine: the compare helper reports

def _perturbed(ref, how):
    rec = T.as_record(ref).copy()
    if how == "one histogram count":
        rec["hist"][0, int(np.argmax(ref["hist"][0]))] += 1
    elif how == "one channel count":
        rec["hist"][3, 255] += 1
    elif how == "one sum + 1":
        rec["sums"][3] += 1
    elif how == "one sum - 1":
        k = int(np.argmax(ref["sums"]))
        rec["sums"][k] -= 1
    elif how == "one rule bound":
        rec["rules"][4, 1] += 1
    elif how == "swapped candidates":
        rec["cand_rule"][[0, 1]] = rec["cand_rule"][[1, 0]]
        rec["cand_invert"][[0, 1]] = rec["cand_invert"][[1, 0]]
        rec["cand_dist"][[0, 1]] = rec["cand_dist"][[1, 0]]
    elif how == "one distance":
        rec["cand_dist"][0] += 1
    elif how == "window origin":
        rec["x1"] += 1
    elif how == "pass":
        rec["pass_"] = 1
    elif how == "unused rule's sum":
        rec["sums"][int(np.argmax(ref["rules"][:, 0] < 0))] = 5
    return rec


@pytest.mark.parametrize("how", ["one histogram count", "one channel count", "one sum + 1", "one sum - 1", "one rule bound",
                                 "swapped candidates", "one distance", "window origin", "pass", "unused rule's sum"])
def test_compare_window_reports_one_perturbed_element(how):
    _, (recs, _, _) = _wc()
    if how == "swapped candidates":
        ref = next(r for r in recs if r["n_cand"] >= 2 and (r["cand_rule"][0], r["cand_dist"][0]) != (r["cand_rule"][1], r["cand_dist"][1]))
    elif how == "unused rule's sum":
        ref = next(r for r in recs if (r["rules"][:, 0] < 0).any())
    else:
        ref = recs[200]
    with pytest.raises(AssertionError):
        T.compare_window(_perturbed(ref, how), ref)


def test_compare_paths_and_before_merge():
    _, (recs, _, _) = _wc()
    from conftest import pkg
    arr = np.array([T.as_record(r, path=i % 3) for i, r in enumerate(recs[:9])], pkg().tail.TRACE_WIN_DTYPE)
    T.compare_paths(arr, {"lds": 3, "canvas": 6, "overflow": 3})
    with pytest.raises(AssertionError):
        T.compare_paths(arr, {"lds": 4, "canvas": 5, "overflow": 3})
    other = arr.copy()
    other["path"] = 1
    assert T.before_merge(arr) == T.before_merge(other)
    other["sums"][4, 2] += 1
    assert T.before_merge(arr) != T.before_merge(other)


# ------------------------------------------------------------------------------------- refine: the launch-shape keys' cases

def test_block_size_case_has_word_counts_on_both_sides_of_every_block_size():
    case = T.block_size_case()
    wins = [T.windows_of(img.shape, boxes) for img, boxes in zip(case["pages"], case["boxes"])]
    assert wins == T.block_size_windows()                                          # the blocks give exactly the intended windows
    tall, (strip,), small = wins
    assert [p.shape[:2] for p in case["pages"]] == [(1030, 360), (4, 8194), (300, 300)]
    one = [(w, h) for _, _, w, h in tall[:9]]
    assert all(w <= 32 for w, _ in one) and [h for _, h in one] == [255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
    three = [(w, h) for _, _, w, h in tall[9:]]
    assert all(65 <= w <= 96 for w, _ in three) and [T.words_of(w, h) for w, h in three] == [255, 258, 513, 1023, 1026]
    assert (strip[2] + 31) >> 5 == 257 and strip[3] == 3                          # wp > 256: no whole row per trip at 256 threads
    assert [(w, h) for _, _, w, h in small] == [(256, 260), (1, 1), (33, 2)]
    words = T.case_words(case)
    assert words == [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 255, 258, 513, 1023, 1026, 771, 2080, 1, 4]
    for nt in T.BLOCK_SIZES:                                                       # both sides of, and exactly, each block size
        assert {nt - 1, nt, nt + 1} <= set(words)
        assert any(wd % 3 == 0 and wd < nt for wd in words[9:14]) and any(wd % 3 == 0 and wd > nt for wd in words[9:14])
        assert nt % 3 != 0
    assert T.words_of(*T.LARGE) > 2048 and (T.words_of(*T.LARGE) + 1) // 2 > T.lds_rcap(T.words_of(*T.LARGE), 1) == 1024   # rlay > rcap at 1
    assert T.large_window_case()["boxes"][0] == [case["boxes"][2][0]] and np.array_equal(T.large_window_case()["pages"][0], case["pages"][2])


@pytest.mark.parametrize("name", ["block_size_case", "class_case"])
def test_launch_shape_cases_fit_their_run_tables_and_reach_the_late_phases(name):
    """By the emulation's run counts (tests/twlds_emul.py) no labelling of any window -- a candidate after the small-component
    rule, or the complement hole filling labels, either refine mode -- has more runs than max(1 024, 2.5 per word): nothing
    overflows at the default `tail_lds_runs_x10`, whatever launch a window shares.  The merge accepts something in at least
    half of the windows and hole filling fills a hole, so the late phases are not compared on empty planes."""
    st = T.merge_stats(getattr(T, name))
    print("\n(words, runs: candidates / complement mode 0 / mode 1, accepted, filled):", [(s["words"], s["runs"], s["accepted"], s["filled"]) for s in st])
    for s in st:
        assert max(s["runs"]) <= max(1024, s["words"] * 25 // 10), s
    assert sum(s["accepted"] > 0 for s in st) * 2 >= len(st)
    assert sum(s["filled"] > 0 for s in st) >= 3
    for mode in (0, 1):
        assert T.expected_paths(getattr(T, name), mode) == {"lds": len(st), "canvas": 0, "overflow": 0}
    if name == "block_size_case":                                                  # the large window completes under the floor of 1 024 runs
        assert max(st[15]["runs"]) <= 1024 and st[15]["words"] == 2080 and st[15]["filled"] > 0
        assert T.expected_paths(T.large_window_case, 1, {"tail_lds_runs_x10": 1}) == {"lds": 1, "canvas": 0, "overflow": 0}
        assert T.expected_paths(T.block_size_case, 0, {"tail_lds_runs_x10": 1})["overflow"] >= 1   # ... while taller columns do overflow there


def test_lds_restatement_against_hand_computed_rows():
    """`lds_rcap`, `lds_need`, `lds_launches` against rows worked out by hand from the layout (3 planes + u16 prefix + parent
    and acc of rlay + 20 words, times 4 bytes) -- not against the library; every key is given, none read from it."""
    rcap, need = T.lds_rcap, T.lds_need
    # 2.5 runs per word.  words = 1: rcap 1 024 (floor), rlay 1 024: (3 + 1 + 2 048 + 20) * 4
    assert (rcap(1, 25), need(1, 25)) == (1024, 8288)
    # words = 600: rcap 1 500, rlay 1 500: (1 800 + 300 + 3 000 + 20) * 4
    assert (rcap(600, 25), need(600, 25)) == (1500, 20480)
    # words = 2 080: rcap 5 200: (6 240 + 1 040 + 10 400 + 20) * 4; at 0.1 runs per word rcap 1 024 < rlay 1 040: (6 240 + 1 040 + 2 080 + 20) * 4
    assert (rcap(2080, 25), need(2080, 25)) == (5200, 70800) and (rcap(2080, 1), need(2080, 1)) == (1024, 37520)
    # words = 4 515 (odd: prefix 2 258 words): rcap 11 287: (13 545 + 2 258 + 22 574 + 20) * 4; 4 516 is the first beyond 150 KB
    assert (rcap(4515, 25), need(4515, 25)) == (11287, 153588) and need(4516, 25) == 153624 > 150 << 10 >= need(4515, 25)
    # 16 runs per word, 100 words: rcap 1 600: (300 + 50 + 3 200 + 20) * 4; 100 per word, 700 words: clamp 65 000
    assert (rcap(100, 160), need(100, 160)) == (1600, 14280)
    assert (rcap(700, 1000), need(700, 1000)) == (65000, (2100 + 350 + 130000 + 20) * 4)
    # `tail_lds_rcap` = 8, 40 words: rlay = 20 (the scratch plane): (120 + 20 + 40 + 20) * 4; the key is clamped as well
    assert (rcap(40, 25, 8), need(40, 25, 8)) == (8, 800) and rcap(40, 25, 70000) == 65000
    # the class loop on class_case's word counts at 40 KB / 80 KB / 150 KB: needs 40 776 <= 40 KB < 44 348 (1 302 words), 70 800 <= 80 KB
    words = [4515, 1, 600, 2080, 40, 600, 1197, 100, 1302, 400, 4]
    assert T.case_words(T.class_case()) == words
    K40, K80, K150 = 40 << 10, 80 << 10, 150 << 10
    assert T.lds_launches(words, K40, K80, K150, 25) == ([], [(8, 1197, 2992, 40776, [1, 10, 4, 7, 9, 2, 5, 6]), (2, 2080, 5200, 70800, [8, 3]),
                                                            (1, 4515, 11287, 153588, [0])])
    # one class: the 1 x 1 window in the layout of the largest
    assert T.lds_launches(words, K150, K150, K150, 25) == ([], [(11, 4515, 11287, 153588, [1, 10, 4, 7, 9, 2, 5, 6, 8, 3, 0])])
    # a limit AT a need keeps the window below, one byte less moves it up; cls1 < cls0 leaves the middle launch out
    assert [l[:2] for l in T.lds_launches(words, 40776, 70800, K150, 25)[1]] == [(8, 1197), (2, 2080), (1, 4515)]
    assert [l[:2] for l in T.lds_launches(words, 40775, 70799, K150, 25)[1]] == [(7, 600), (2, 1302), (2, 4515)]
    assert [l[:2] for l in T.lds_launches(words, K80, K40, K150, 25)[1]] == [(10, 2080), (1, 4515)]
    assert [l[:2] for l in T.lds_launches(words, 0, K80, K150, 25)[1]] == [(10, 2080), (1, 4515)]
    # 16 runs per word: need 142 w + 80 -> 1 081 words is the last in LDS; the others take the canvases, in window order
    assert T.lds_launches(words, K40, K80, K150, 160)[0] == [0, 3, 6, 8] and T.lds_launches(words, K40, K80, K150, 25, lds=0) == (list(range(11)), [])
    # a lower LDS limit sends the largest to the canvases
    assert T.lds_launches(words, K40, K80, 153587, 25)[0] == [0]


def test_class_settings_move_windows_between_launches():
    words = T.case_words(T.class_case())
    assert len(words) == 11 and sorted(words)[0] == 1 and sorted(words).count(600) == 2 and max(words) == 4515
    shapes = {what: [l[:2] for l in T.launches_of_setting(words, tune)[1]] for what, tune in T.class_settings()}
    assert len({str(v) for v in shapes.values()}) >= 6, shapes                     # the settings differ in what they launch
    assert shapes["one class"] == [(11, 4515)]
    assert shapes["the two 600-word windows a launch of their own"] == [(5, 400), (2, 600), (4, 4515)]
    assert shapes["the 1 x 1 window alone, then all but the largest"] == [(1, 1), (9, 2080), (1, 4515)]
    assert shapes["both one byte below"] != shapes["cls0 at the need of the 1 197-word window, cls1 at that of the 2 080-word one"] == shapes["the defaults"]
    assert all(T.launches_of_setting(words, tune)[0] == [] for _, tune in T.class_settings())


def test_compare_launches_reports():
    launches = T.lds_launches([600, 1, 2080], 40 << 10, 80 << 10, 150 << 10, 25)[1]
    got = [dict(windows=n, max_words=mw, rcap=rc, bytes=by, threads=512, refused=0) for n, mw, rc, by, _ in launches]
    T.compare_launches(got, (launches, 512))
    for k in ("windows", "max_words", "rcap", "bytes", "threads", "refused"):
        bad = [dict(g) for g in got]
        bad[-1][k] += 1
        with pytest.raises(AssertionError):
            T.compare_launches(bad, (launches, 512))
    with pytest.raises(AssertionError):
        T.compare_launches(got[:-1], (launches, 512))


# ------------------------------------------------------------------------------------------------------------------- DB stage

def test_db_calls_cover_the_listed_maps():
    calls = T.db_calls()
    maps = {name: pr for _, call in calls for name, pr in call}
    for name in ("holes", "thin", "empty", "full", "cap", "frame", "speckle 0", "speckle 1", "speckle 3", "1 x 1 set", "1 x 40", "40 x 1",
                 "31 x 31", "32 x 32", "33 x 33", "overflow"):
        assert name in maps, name
    assert all(len({pr.shape for _, pr in call}) == 1 for _, call in calls)      # one shape per call
    assert sum(len(call) >= 3 and len({pr.tobytes() for _, pr in call}) == len(call) for _, call in calls) >= 2   # batch offsets
    nf, nb = T.db_counts(maps["overflow"])
    assert nf > T.COMP_CAP                                                         # by the emulation's own count


@functools.lru_cache(None)
def _db_ref(name):
    maps = {n: pr for _, call in T.db_calls() for n, pr in call}
    return T.db_reference(maps[name])


def _as_got(ref):
    rows = ref["rows"]
    got = {k: np.array(ref[k]).copy() for k in T._INT_TABLES + ("sum_f", "sum_b", "ring_sum")}
    got["row_lo"], got["row_hi"] = np.array(ref["row_lo"][:rows]).copy(), np.array(ref["row_hi"][:rows]).copy()
    got["hdr"] = np.array([ref["n_f"], ref["n_b"], rows, 0], np.int32)
    return got


def test_db_references_are_not_vacuous():
    holes, cap, sp = _db_ref("holes"), _db_ref("cap"), _db_ref("speckle 1")
    assert (holes["par_b"] > 0).sum() == 2 and (holes["ring_cnt"] > 0).sum() == 2 and (holes["par_f"] > 0).sum() >= 2
    assert cap["n_f"] > 1000 and sp["n_b"] > 100 and (sp["par_b"] > 0).sum() > 50
    for t in (holes, cap, sp, _db_ref("33 x 33"), _db_ref("1 x 1 set")):
        rows = t["rows"]
        assert (t["row_lo"][:rows] <= t["row_hi"][:rows]).all()                   # every row of every component and ring is touched
        for k in ("sum_f", "sum_b", "ring_sum"):                                  # bounds: derived, tiny, and 0 only where nothing is added
            b = t["bound_" + k]
            assert (b >= 0).all() and (b <= 1e-11 * np.maximum(np.abs(t[k]), 1e-3) + 1e-300).all(), (k, float(b.max()))
        T.compare_db_tables(_as_got(t), t)
    assert (holes["bound_sum_f"] > 0).all() and (holes["bound_sum_f"] < 0.05 * 1e-6).all()   # far below one pixel's probability


@pytest.mark.parametrize("how", ["one row_lo", "one row_hi", "one ring_cnt", "one sum_f beyond its bound", "one ring_sum beyond its bound",
                                 "one sum_b beyond its bound", "one off_b", "one par_f", "hdr rows", "one first_f", "overflow flag"])
def test_compare_db_tables_reports_one_perturbed_element(how):
    ref = _db_ref("holes")
    got = _as_got(ref)
    T.compare_db_tables(got, ref)
    hole = int(np.argmax(ref["par_b"] > 0))
    if how == "one row_lo":
        got["row_lo"][ref["rows"] // 2] += 1
    elif how == "one row_hi":
        got["row_hi"][ref["rows"] - 1] -= 1
    elif how == "one ring_cnt":
        got["ring_cnt"][hole] += 1
    elif how == "one sum_f beyond its bound":
        got["sum_f"][1] += 3 * ref["bound_sum_f"][1]
    elif how == "one ring_sum beyond its bound":
        got["ring_sum"][hole] -= 3 * ref["bound_ring_sum"][hole]
    elif how == "one sum_b beyond its bound":
        got["sum_b"][hole] += 3 * ref["bound_sum_b"][hole]
    elif how == "one off_b":
        got["off_b"][-1] += 1
    elif how == "one par_f":
        got["par_f"][0] += 1
    elif how == "hdr rows":
        got["hdr"][2] += 1
    elif how == "one first_f":
        got["first_f"][2] += 1
    elif how == "overflow flag":
        got["hdr"][3] = 1
    with pytest.raises(AssertionError):
        T.compare_db_tables(got, ref)


def test_sums_inside_their_bounds_pass_and_one_pixel_less_does_not():
    """The bound is orders of magnitude below what the issue's corruption changes: one pixel left out of one sum_f."""
    ref = _db_ref("speckle 3")
    got = _as_got(ref)
    got["sum_f"] = got["sum_f"] + 0.9 * ref["bound_sum_f"]
    T.compare_db_tables(got, ref)
    k = int(np.argmax(ref["st_f"][:, 4]))
    p = ref["first_f"][k]
    got["sum_f"][k] -= float(_maps("speckle 3").ravel()[p])
    with pytest.raises(AssertionError):
        T.compare_db_tables(got, ref)


def _maps(name):
    return {n: pr for _, call in T.db_calls() for n, pr in call}[name]


def test_overflow_is_decided_by_the_emulation_alone():
    """A device that raised the flag on a map that fits is reported; on the map that does not fit only the flag is compared."""
    nf, nb = T.db_counts(_maps("overflow"))
    over = dict(n_f=nf, n_b=nb, rows=nf)
    T.compare_db_tables({"hdr": np.array([T.COMP_CAP, nb, 0, 1], np.int32)}, over)
    with pytest.raises(AssertionError):
        T.compare_db_tables({"hdr": np.array([T.COMP_CAP, nb, 0, 0], np.int32)}, over)


# ------------------------------------------------------------------------------------------------------------ the record's layout

def test_trace_window_record_has_the_c_layout():
    """`tail.TRACE_WIN_DTYPE` / `_lib.CtdTraceWin` against `ctd_trace_win` of the header, compiled: size and every offset."""
    import ctypes as C
    from c_layout import compiled_flat
    from conftest import pkg
    p = pkg()
    names = ["page", "x1", "y1", "w", "h", "pass", "path", "n_cand", "hist", "rules", "cand_rule", "cand_invert", "sums", "cand_dist"]
    vals = compiled_flat({"ctd_trace_win": names})
    dt, W = p.tail.TRACE_WIN_DTYPE, p._lib.CtdTraceWin
    py = ["pass_" if n == "pass" else n for n in names]
    assert vals == [dt.itemsize] + [dt.fields[n][1] for n in py] == [C.sizeof(W)] + [getattr(W, n).offset for n in py]
