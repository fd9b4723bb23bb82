"""ilqg.py and problem libraries built before ilqg_batch_shift / ilqg_batch_receding / ilqg_multi_shift existed (a pair
compiled out of tree and not rebuilt since): such a library still loads — load_library binds the receding-horizon entries
only where the library exports them — and the methods that need them say what to do."""
import pytest

from conftest import load_package


class OldLibrary:
    """stands for a CDLL without the receding-horizon symbols"""


@pytest.mark.parametrize("name", ["ilqg_batch_shift", "ilqg_batch_receding", "ilqg_multi_shift"])
def test_missing_receding_entry_is_a_clear_error(name):
    ilqg = load_package().ilqg
    with pytest.raises(ilqg.IlqgError) as e:
        ilqg._receding_entry(OldLibrary(), name)
    assert name in str(e.value) and "rebuild" in str(e.value)


def test_present_receding_entry_is_returned():
    ilqg = load_package().ilqg
    lib = OldLibrary()
    lib.ilqg_batch_shift = object()
    assert ilqg._receding_entry(lib, "ilqg_batch_shift") is lib.ilqg_batch_shift
