#!/usr/bin/env python3
"""Registers, scratch and LDS of every kernel in a device assembly file (hipcc --cuda-device-only -S): what to look at
after touching a kernel - a private segment > 0 means spills or a dynamically indexed register array.

    kernel_resources.py FILE.s [substring]            the table
    kernel_resources.py --compare OLD.s NEW.s         every kernel of the two files put into one class:
        identical    the same instruction text (block labels apart from the function's number in the file)
        reordered    equal VGPR, AGPR, scratch, spills and LDS and equal per-mnemonic instruction counts (SGPRs may differ)
        DIFFERENT    anything else, with what differs; also a kernel that only one file has
        --rename OLD=NEW (repeatable, after the two files): the one kernel of OLD.s whose name contains OLD is paired with
        the one of NEW.s whose name contains NEW, and listed as OLD=NEW
    --compare exits with status 1 when a kernel is DIFFERENT."""
import collections
import re
import sys

KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")
SHORT = ("vgpr", "agpr", "sgpr", "scratch", "spill", "lds")


def resources(txt):
    """kernel name -> {key: value} from the metadata at the end of the file"""
    out = {}
    for blk in txt.split("- .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        g = lambda k: (re.search(r"\.%s:\s*(\S+)" % k, blk) or [None, "?"])[1]
        out[g("name")] = {k: g(k) for k in KEYS}
    return out


def bodies(txt, names):
    """kernel name -> its instruction lines (labels, directives and comments dropped)"""
    out = {}
    lines = txt.split("\n")
    starts = {l.split(":")[0]: i for i, l in enumerate(lines) if l[:1] == "_" and l.split(":")[0] in names}
    for name, i in starts.items():
        body = []
        for l in lines[i + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";")[0].strip()
            if l and not l.startswith(".") and not l.endswith(":"):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", l)))   # block labels carry the function's number in the file
        out[name] = body
    return out


def table(path, pat):
    for name, r in resources(open(path).read()).items():
        if pat and pat not in name:
            continue
        print("%-100s " % name[:100] + " ".join("%s %s" % (s, r[k]) for s, k in zip(SHORT, KEYS)))


def compare(old_path, new_path, renames=()):
    old_txt, new_txt = open(old_path).read(), open(new_path).read()
    ro, rn = resources(old_txt), resources(new_txt)
    bo, bn = bodies(old_txt, ro), bodies(new_txt, rn)
    for pair in renames:
        for sub, r, b in zip(pair.split("="), (ro, rn), (bo, bn)):
            name, = [k for k in r if sub in k and "=" not in k]                      # exactly one kernel, not yet paired
            r[pair], b[pair] = r.pop(name), b.pop(name)
    bad = 0
    for name in sorted(set(ro) | set(rn)):
        if name not in ro or name not in rn:
            print("DIFFERENT  %s: only in %s" % (name, old_path if name in ro else new_path))
            bad += 1
            continue
        if bo[name] == bn[name]:
            print("identical  %s" % name)
            continue
        why = ["%s %s -> %s" % (s, ro[name][k], rn[name][k]) for s, k in zip(SHORT, KEYS) if k != "sgpr_count" and ro[name][k] != rn[name][k]]
        co, cn = (collections.Counter(l.split(" ")[0] for l in b[name]) for b in (bo, bn))
        why += ["%s x%d -> x%d" % (m, co[m], cn[m]) for m in sorted(set(co) | set(cn)) if co[m] != cn[m]]
        if why:
            print("DIFFERENT  %s: %s" % (name, ", ".join(why)))
            bad += 1
        else:
            print("reordered  %s (sgpr %s -> %s)" % (name, ro[name]["sgpr_count"], rn[name]["sgpr_count"]))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        assert len(sys.argv) % 2 == 0 and set(sys.argv[4::2]) <= {"--rename"}, __doc__
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[5::2]))
    table(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
