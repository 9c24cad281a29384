"""The one loader behind api.load_library and its four siblings, on the CPU: the default path is loaded once and cached, an
explicit path is loaded anew and leaves the cached instance alone, a missing library is a FileNotFoundError that says how to build it."""
import shutil

import pytest

LOADERS = {"load_library": "LIB_PATH", "load_host_library": "HOST_LIB_PATH", "load_circ_library": "CIRC_LIB_PATH",
           "load_cols_library": "COLS_LIB_PATH", "load_vals_library": "VALS_LIB_PATH"}


@pytest.mark.parametrize("loader", LOADERS)
def test_default_is_cached_and_an_explicit_path_is_not(pkg, tmp_path, loader):
    load, path = getattr(pkg.api, loader), getattr(pkg.api, LOADERS[loader])
    first = load()
    assert load() is first
    # a copy finds libaesw.so already mapped (its $ORIGIN no longer holds one): the loader maps that first
    copy = shutil.copy(path, tmp_path / path.name)
    other = load(copy)
    assert other is not first and load(copy) is not other
    assert load() is first
    symbols = getattr(pkg.api, LOADERS[loader].replace("LIB_PATH", "SYMBOLS"))
    assert all(getattr(other, name).restype is res for name, (res, _args) in symbols.items())  # the copy's symbols are bound as well


@pytest.mark.parametrize("loader", LOADERS)
def test_a_missing_library_says_how_to_build_it(pkg, tmp_path, loader):
    missing = tmp_path / "nowhere" / getattr(pkg.api, LOADERS[loader]).name
    with pytest.raises(FileNotFoundError) as e:
        getattr(pkg.api, loader)(missing)
    assert str(missing) in str(e.value) and "import __graft_entry__ as g; g.build()" in str(e.value)
    assert ("There is no fallback implementation." in str(e.value)) == (loader != "load_host_library")
