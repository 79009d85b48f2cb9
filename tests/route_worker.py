"""Child process of tests/test_gpu_route_matrix.py test_every_reachable_instantiation_is_rendered: the route matrix's renders (every route, every schedule,
whole image and tiles; no oracle) on cuda:0.  The parent starts it with NRS_DEV_KNOBS=1 NRS_KERNEL_LOG=1 and reads the "[nrs kernel]" lines off its stderr.
usage: route_worker.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import test_gpu_route_matrix as rm
    rigs = rm.Rigs()
    for route in rm.ROUTES:
        rm.render_route(rigs, route, oracle=False)
        sys.stderr.flush()
    print(f"routes rendered: {len(rm.ROUTES)}", flush=True)


if __name__ == "__main__":
    main()
