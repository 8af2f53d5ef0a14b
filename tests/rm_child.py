"""Child process of tests/test_rm_sweep_gpu.py::test_decode_with_dense_writes_in_child: MI355_RM_SPARSE is read once
per process, so the decodes with dense writes run here; results go to the .npz named on the command line."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

if __name__ == "__main__":
    import test_rm_sweep_gpu

    test_rm_sweep_gpu._child_main(sys.argv[1])
