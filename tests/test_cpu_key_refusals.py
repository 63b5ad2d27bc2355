"""What every keyed C-ABI entry point and the two row-update forms refuse, status and fr_last_error() text, and what a status word's bits are reported
as, on the CPU back-end (device = -1): tests/key_refusals.py against the `cpu` section of tests/golden/key_refusals.json.  Runs without a GPU;
tests/test_gpu_key_refusals.py runs the same tables on the MI355X."""
import key_refusals as KR


def test_the_case_table_is_whole():
    KR.check_table_is_whole()


def test_refusals_and_status_texts_keep_their_status_text_and_order(fr):
    KR.check_refusals(fr, KR.CPU)
