"""ds_read_b128 bank-conflict check of the LDS layouts of conv_s2w.hip (stem 8x8/s2 as space-to-depth F(2x2,4x4)), with the
lane groups of tools/lds_bank_check.py.  A wave owns 2 x 8 blocks of 2 x 2 outputs; a lane (r16, kq) reads quad kq of the
5 x 5 cells of block r16, and quad kq of weight row r16 of the slab.  Prints the worst number of distinct addresses that share a
bank slot within one lane group (1 = conflict-free) for every read of the sweep."""

G = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
     list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
G += [[l + 32 for l in g] for g in G]

PW = 19                 # patch cells per row (16 outputs + 3)
SY = PW * 4 + 2         # row stride in quads (conv_s2w.hip)


def conflicts(addr_fn):
    worst = 0
    for g in G:
        slots = {}
        for l in g:
            a = addr_fn(l)
            slots.setdefault(a % 16, set()).add(a)
        worst = max(worst, max(len(s) for s in slots.values()))
    return worst


def pslot(px, quad):
    return px * 4 + ((quad + 2 * (px >> 2)) & 3)


def wslot(row, quad):
    return row * 4 + ((quad + (row >> 1)) & 3)


def check_patch():
    worst = 0
    for r in range(5):
        for c in range(5):
            for wave in range(4):
                def addr(l):
                    r16, kq = l & 15, l >> 4
                    br, bc = r16 >> 3, r16 & 7
                    return (wave * 4 + 2 * br + r) * SY + pslot(2 * bc + c, kq)
                worst = max(worst, conflicts(addr))
    return worst


def check_slab():
    return conflicts(lambda l: wslot(l & 15, l >> 4))


if __name__ == "__main__":
    p, w = check_patch(), check_slab()
    print(f"patch (row stride {SY} quads): {p}   weight slab: {w}")
    raise SystemExit(0 if p == 1 and w == 1 else 1)
