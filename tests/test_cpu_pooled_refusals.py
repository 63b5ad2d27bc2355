"""What every pooled C-ABI entry point refuses, status and fr_last_error() text, on the CPU back-end (device = -1): tests/pooled_refusals.py against the
`cpu` section of tests/golden/pooled_refusals.json.  Runs without a GPU; tests/test_gpu_pooled_refusals.py runs the same table on the MI355X."""
import pooled_refusals as PR


def test_the_case_table_is_whole():
    PR.check_table_is_whole()


def test_refusals_keep_their_status_text_and_order(fr):
    PR.check_refusals(fr, PR.CPU)
