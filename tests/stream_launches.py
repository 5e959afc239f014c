"""mpx_timing.launches of the SDMA engine's loopback pairs, as literals.

One per copy, signal or wait enqueued for the call (none for a zero-byte
copy), one per graph replay; checksums, fills and receive accounting are not
counted.  Read off the engine's loops by hand; tests/test_gpu_engine.py holds
the GPU against them, tests/test_tools.py the CPU trace of the shared loop
(tools/stream_loop_check.cpp) plus the handshake and replay terms below.
"""
PINGPONG, NONBLOCKING, UNIDIR = 0, 1, 2
SIZES = [0, 1, 4097]
# (iters, check): below the graph minimum of 16 unchecked (plain enqueue);
# around one window checked (check mode never replays graphs); 600 unchecked:
# two replayed 256-iteration chunks and a captured remainder of 88
SHAPES = [(1, False), (3, False), (15, False), (255, True), (256, True), (257, True), (600, False)]
GRAPH_MIN, CHUNK = 16, 256

# (pull, mode, payload copies happen: n > 0) -> per shape, (group 1's, group 0's)
LAUNCHES = {
    (False, PINGPONG, False): [(4, 3), (8, 7), (32, 31), (512, 511), (514, 513), (516, 515), (5, 4)],
    (False, PINGPONG, True): [(5, 4), (11, 10), (47, 46), (767, 766), (770, 769), (773, 772), (5, 4)],
    (False, NONBLOCKING, False): [(4, 4), (4, 4), (4, 4), (767, 767), (770, 770), (774, 774), (6, 6)],
    (False, NONBLOCKING, True): [(5, 5), (7, 7), (19, 19), (1022, 1022), (1026, 1026), (1031, 1031), (6, 6)],
    (False, UNIDIR, False): [(4, 4), (8, 10), (32, 46), (512, 766), (514, 769), (516, 772), (5, 4)],
    (False, UNIDIR, True): [(5, 4), (11, 10), (47, 46), (767, 766), (770, 769), (773, 772), (5, 4)],
    (True, PINGPONG, False): [(6, 5), (12, 11), (48, 47), (768, 767), (771, 770), (774, 773), (6, 5)],
    (True, PINGPONG, True): [(7, 6), (15, 14), (63, 62), (1023, 1022), (1027, 1026), (1031, 1030), (6, 5)],
    (True, NONBLOCKING, False): [(6, 6), (10, 10), (34, 34), (529, 529), (533, 533), (536, 536), (6, 6)],
    (True, NONBLOCKING, True): [(7, 7), (13, 13), (49, 49), (784, 784), (789, 789), (793, 793), (6, 6)],
    (True, UNIDIR, False): [(5, 5), (9, 13), (33, 61), (513, 1021), (515, 1025), (517, 1029), (6, 4)],
    (True, UNIDIR, True): [(5, 6), (9, 16), (33, 76), (513, 1276), (515, 1281), (517, 1286), (6, 4)],
}


def launches(pull, mode, group, n, iters, check):
    return LAUNCHES[(pull, mode, n > 0)][SHAPES.index((iters, check))][0 if group == 1 else 1]


def replayed(iters, check):
    """(graph replays, iterations they cover) of an unchecked call"""
    if check or iters < GRAPH_MIN:
        return 0, 0
    rest = iters % CHUNK if iters % CHUNK >= GRAPH_MIN else 0
    return iters // CHUNK + (1 if rest else 0), iters - iters % CHUNK + rest


def handshake(mode, group, iters):
    """the call's 'receives posted' store, and the wait for the peer's by a
    side that pushes first"""
    return 0 if iters == 0 else 1 + (1 if (mode == NONBLOCKING or group == 1) else 0)
