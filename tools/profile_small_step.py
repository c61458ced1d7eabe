import time, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cyclistsocialforce_amd.vehicle import TwoDBicycle
from cyclistsocialforce_amd.intersection import SocialForceIntersection
a = TwoDBicycle((-6, 0, 0, 5, 0), id="a"); b = TwoDBicycle((15, -20, np.pi/2, 5, 0), id="b"); c = TwoDBicycle((13, -20, np.pi/2, 5, 0), id="c")
a.setDestinations((35, 64, 65), (0, 0, 0)); b.setDestinations((15, 15, 15), (20, 49, 50)); c.setDestinations((13, 13, 13), (20, 49, 50))
ins = SocialForceIntersection((a, b, c))
for _ in range(50): ins.step()
e = ins.engine
def t(f, n=300):
    t0 = time.perf_counter()
    for _ in range(n): f()
    return (time.perf_counter() - t0) / n * 1e6
print("step() total        %.1f us" % t(ins.step))
print("_push_mutations     %.1f us" % t(ins._push_mutations))
print("engine.step(1)      %.1f us" % t(lambda: e.step(1)))
e.sync()
print("engine.step(1)+sync %.1f us" % t(lambda: (e.step(1), e.sync())))
print("state(with_nav)     %.1f us" % t(lambda: e.state(with_nav=True)))
print("forces()            %.1f us" % t(e.forces))
print("_pull               %.1f us" % t(lambda: ins._pull(True, 1)))
import cProfile, pstats
pr = cProfile.Profile(); pr.enable()
for _ in range(300): ins.step()
pr.disable(); pstats.Stats(pr).sort_stats("cumulative").print_stats(14)
