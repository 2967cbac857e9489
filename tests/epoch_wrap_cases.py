"""The schedules of tests/test_gpu_epoch_wrap.py, as data (no torch, no device): which step of a run senses at which claim epoch,
the orders in which five kinds of step take turns on one batch around the wrap, and the steps at which a stand-alone agent
senses while something else drives its world.  tests/test_epoch_wrap_cases_cpu.py checks that the tables do what they claim.

The epoch tag runs 1 .. EPOCH_MAX and starts over: step i of a run from a fresh world (i = 0, 1, ...) senses at
`sense_epoch(i)` = i % 31 + 1 and claims at the next one, so steps i and i + 31 sense under the same tag."""
EPOCH_MAX = 31                       # die_amd._lib.OWNER_EPOCH_MAX (the GPU file asserts the two agree)


def sense_epoch(i: int) -> int:
    """The epoch step i of a run from a fresh world senses at."""
    return i % EPOCH_MAX + 1


# ------------------------------------------------------------------------------------------------ reaching the wrap
WARM_UP = 28                         # real steps before a window: the window's first link senses at epoch 29
WINDOW = 5                           # links of a gradient window: sense epochs 29, 30, 31, 1, 2
LINKS_AT = (29, 30, 31, 32)          # the steps of the link-by-link comparison: sense epochs 30, 31, 1, 2
POPULATION_STEPS = 40                # a population's run: sense epochs 1 .. 31, then 1 .. 9
SAME_AS_FORWARD_STEPS = 34           # `recurrent_action` / `signalling_action` against `forward`: sense epochs 1 .. 31, 1, 2, 3
SECOND_CYCLE = {e: (e - 1, e - 1 + EPOCH_MAX) for e in (1, 2)}    # epoch -> (the step that senses at it first, the step that does again)
MOVED_ON = (31, 62)                  # steps between a graph's last link and its backward: the tags have come round once, twice

# ------------------------------------------------------------------------------------------------ taking turns (group 3)
# S: signal population, M: memory population, K: stock population — the BUILDERS, whose step builds the batch's stock / standing
# planes at its sense epoch; P: plain population, A: step_action — the others, after which the next builder must start the planes
# over.  An order is read left to right, one letter a step; letter i steps at sense_epoch(i).
KINDS = 'SMKPA'
BUILDERS = 'SMK'
OTHERS = 'PA'
AT_30, AT_31, AT_1 = 29, 30, 31      # the steps that sense at epochs 30, 31 and 1 (of the second cycle)
ORDER_STEPS = 35                     # sense epochs 1 .. 31, then 1 .. 4

# Words of the first cycle survive up to the wrap only where no step in between made the batch start the planes over: then the
# library's clear at sense epoch 31 alone stands between a word tagged 1 and the builder that reads at epoch 1 again.
ALL_BUILDERS = 'SMK' * 10            # 30 steps, every one a builder: the prefix of the orders whose steps at 30 and 31 are builders
# … and everywhere else the five kinds take turns from the start; builders at steps 0 and 1 write the words tagged 1 and 2.
MIXED = 'SKMPASMKAPKSMPPMAKSASKMPMAKSP'[:AT_30]


def _order(at_30: str, at_31: str, at_1: str) -> str:
    prefix = ALL_BUILDERS[:AT_30] if at_30 in BUILDERS and at_31 in BUILDERS else MIXED
    tail = {'S': 'MKS', 'M': 'KSM', 'K': 'SMK', 'P': 'SMK', 'A': 'KSM'}[at_1]      # a builder reads at epoch 2, whoever stepped at 1
    return prefix + at_30 + at_31 + at_1 + tail


# every triple (builder, other, builder) at sense epochs 30, 31, 1 …
_TRIPLES = [(b, n, c) for b in BUILDERS for n in OTHERS for c in BUILDERS]
# … and every ordered pair at sense epochs 31, 1 that those triples do not hold, behind a step at 30 that varies with the pair
_PAIRS = [(x, y) for x in KINDS for y in KINDS if not (x in OTHERS and y in BUILDERS)]
ORDERS = [_order(*t) for t in _TRIPLES] + [_order(KINDS[(KINDS.index(x) + KINDS.index(y)) % 3], x, y) for x, y in _PAIRS]

# ------------------------------------------------------------------------------------------------ irregular forwards (group 4)
# A stand-alone agent owns its standing plane and starts it over when the epoch it builds at is not greater than the epoch of its
# last build.  The agent senses at these steps only (a repeated step: twice without a step in between); something else drives the
# world.  Gaps 0, 1, 30, 31, 32, 62.
SENSE_AT = (0, 0, 1, 31, 62, 94, 156)
GAPS = (0, 1, 30, 31, 32, 62)
# what the rule distinguishes, by the pair (gap, how the new epoch compares with the last build's): the sense at SENSE_AT[j + 1]
RELATIONS = ('equal, no step between', 'higher, same cycle', 'lower', 'equal, one cycle later', 'higher, next cycle', 'equal, two cycles later')
# the pairs (earlier sense, later sense) whose builds carry one tag with a whole cycle or more between them: a word of the earlier
# build left in the plane would read as an agent at the later one
SAME_TAG = ((0, 31), (31, 62), (94, 156))
