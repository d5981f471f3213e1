"""The rule of match_finder="auto" against libzstd, on the CPU: per data set of tests/auto_model.py the totals under "none" everywhere, level 3 everywhere, the better of
the two per frame and the model's choice, the regret against the better per frame, and every frame the model got wrong -- for seed 1 (the seed the constants were
chosen on) and seed 2 (which they never saw).  python tests/tools/auto_finder_rule.py > profiles/r17_auto_finder_rule.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import auto_model as am, reflib      # noqa: E402

ref = reflib.checker()
print("match_finder=\"auto\": the model's choice (tests/auto_model.py) against libzstd 1.5.7's two sizes per frame (%s)" % reflib.REF_KIND.split(" (")[0])
print("constants: MIN %d ALL %d windows %d x %d feed %d stride %d table 2^%d cap %d sequence %d bits + log2 offset, search where credit * %d > literal bits * %d"
      % (am.MIN, am.ALL, am.NWIN, am.WIN, am.FEED, am.STRIDE, am.HLOG, am.CAP, am.SEQ_BITS, am.DEN, am.NUM))
for seed in (1, 2):
    print("\nseed %d (text: frames %d ... %d of the bench corpus)" % (seed, 24 * (seed - 1), 24 * seed - 1))
    print("%-26s %6s %10s %10s %10s %10s %8s %6s" % ("set", "frames", "all none", "all lvl 3", "best/frame", "auto", "regret", "wrong"))
    wrong = []
    for name, frames in am.data_sets(seed):
        tn = tl = tb = ta = 0
        nw = 0
        for i, f in enumerate(frames):
            nn, l3 = am.both_sizes(ref, f)
            ch, st = am.classify(f)
            tn += nn; tl += l3; tb += min(nn, l3); ta += nn if ch == am.LITERALS else l3
            if (ch == am.LITERALS and l3 < nn) or (ch == am.SEARCH and nn <= l3):
                nw += 1
                wrong.append("  %-26s frame %2d: none %7d level 3 %7d chose %s (credit / literal bits %.4f, %d hits in %d sampled bytes)"
                             % (name, i, nn, l3, "none" if ch else "the search", st[2] / max(1, st[1]), st[3], st[0]))
        print("%-26s %6d %10d %10d %10d %10d %8d %6d" % (name, len(frames), tn, tl, tb, ta, ta - tb, nw))
    print("frames where the other finder was smaller (or as small and cheaper):")
    print("\n".join(wrong) if wrong else "  none")
