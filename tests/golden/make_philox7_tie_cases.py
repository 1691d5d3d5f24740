"""Search the first seed of every fixed case of tests/test_gpu_philox_rounds.py and write tests/golden/philox7_tie_cases.json
-- TEST INFRASTRUCTURE, numpy and the CPU oracle's initial configurations only.

Philox4x32-7 draws other words than Philox4x32-10, so the quads with many ties that tests/golden/make_tie_cases.py found for ten
rounds say nothing about seven.  Per kernel group (philox_rounds_reference.GROUPS) and coupling this script takes the smallest
seed >= 1 for which the seven-round reference trajectory of the group's cases (that seed beside two fixed ones, the betas of
UNIFORM then PER_REPLICA) holds at least one tie in each costly class and one quad with five or more ties: the second tie call.

    python tests/golden/make_philox7_tie_cases.py

The result is a function of the reference alone; tests/test_philox_rounds_host.py recounts it."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import numpy as np  # noqa: E402

import lat_variants_reference as LV  # noqa: E402
import philox_rounds_reference as PR  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    seeds, found = {}, {}
    for group in PR.GROUPS:
        seeds[group], found[group] = {}, {}
        for coupling in LV.COUPLINGS:
            for seed in range(1, 100000):
                trial = np.array([seed, int(LV.SEEDS[1]), int(LV.SEEDS[2])], dtype=np.uint64)
                n3, n4, most = PR.coverage(O, group, coupling, 7, trial)
                PR._RUNS.clear()
                if n3 >= 1 and n4 >= 1 and most >= 5:
                    seeds[group][coupling] = seed
                    found[group][coupling] = {"class3_ties": n3, "class4_ties": n4, "most_ties_in_a_quad": most}
                    print(group, coupling, seed, found[group][coupling], flush=True)
                    break
            else:
                raise SystemExit(f"no seed for {group} {coupling}")
    with open(PR.GOLDEN, "w") as f:
        json.dump({"generator": "tests/golden/make_philox7_tie_cases.py", "rounds": 7, "seeds": seeds, "found": found}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
