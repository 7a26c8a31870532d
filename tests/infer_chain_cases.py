"""Shapes and builders shared by tests/test_gpu_infer_chain.py and tests/test_host_infer_chain.py: the fused
last two blocks of `infer` are held to the unfused path bit for bit, so a case is a model of tests/infer_cases.py (the
same builders, parameters and inputs) and a number of rows."""
import infer_cases as ic

def blocks(case):
    """Linear blocks of a case: the MAG layout's first layer is the embedding, which `infer` does not run."""
    return case[5] if case[1] == "model" else case[5] - 1


# every case of infer_cases with at least two blocks, then BITWISE's multi-block ones.  pubmed and aminer have one block,
# and so has "mag" (MAG layout, two layers: the embedding and one Linear, 64 -> 8), which `infer(fused=True)` has to
# refuse: ONE_BLOCK.  "deep" and "mag_bn" have three blocks: the first one unfused, the last pair fused
ONE_BLOCK = [c for c in ic.CASES if blocks(c) < 2]
CASES = [c for c in ic.CASES if blocks(c) >= 2] + [c for c in ic.BITWISE if c not in ic.CASES and blocks(c) >= 2]
ROWS = (1, 31, 32, 33, 63, 64, 65, 129, 300)                 # every edge of the 32-, 64- and 128-row tiles

B = 70                                                       # rows of the flag, hidden, class and reduction edges
FLAG_SHAPES = [(7, 33, 5), (100, 1024, 47)]
FLAG_SETS = [(bn, norm) for bn in (False, True) for norm in (False, True)]
HIDDEN_EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1000, 1023, 1024)
CLASS_EDGES = (1, 16, 17, 47, 48, 49, 64)
EDGE_F_IN = 17
K_EDGES = (1, 3, 15, 16, 17, 33, 100, 602)                   # f_in at H = 130, C = 5

RULE_CASES = ("amazon2m", "reddit")
RULE_ROWS = 129

CHUNK = ("chunk", "model", 7, 33, 5, 3, True, True)          # three blocks, B = 300
CHUNK_ROWS = 300
MAG_LARGE = ("mag70k", "mag", 64, 64, 8, 3, False, False)     # the MAG layout with two blocks: 64 -> 64 -> 8
LARGE_ROWS = 70001
AMAZON = next(c for c in ic.CASES if c[0] == "amazon2m")
MEMORY_ROWS = 20000


def two_block(F, H, C, use_bn=True, node_norm=True):
    return (f"{F}-{H}-{C}", "model", F, H, C, 2, use_bn, node_norm)


def model(case, seed=0):
    """Ours on the CPU, built as infer_cases.pair builds it."""
    return ic.pair(case, seed)[0]
