"""A pure-Python model of the search for a batch's invalid tuples (csrc/host_find.hip): the level loop
over find_split and find_next_level, with the pairing replaced by a predicate on ranges.  split and
next_level are the functions under test (tests/findprobe.py) or any stand-ins with the same form."""
import bisect


def search(n, F, max_bad, passes, split, next_level):
    """-> (bad indices ascending, more, levels); passes(lo, hi): the range holds no invalid tuple.
    F: the fan-out, or a function of a level's suspects that gives it (find_level_fanout)."""
    suspects, bad, more, levels = ([(0, n)] if n else []), [], False, 0
    while suspects:
        f = F(suspects) if callable(F) else F
        parts = [p for lo, hi in suspects for p in split(lo, hi, f)]
        verdicts = [passes(lo, hi) for lo, hi in parts]
        suspects, bad, more = next_level(parts, verdicts, max_bad, bad, more)
        levels += 1
    return bad, more, levels


def contains(bad):
    """the predicate of a set of invalid indices"""
    s = sorted(bad)

    def passes(lo, hi):
        i = bisect.bisect_left(s, lo)
        return not (i < len(s) and s[i] < hi)
    return passes
