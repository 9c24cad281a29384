"""The one loader behind api.load_library and its fourteen siblings, on the CPU: the default path is loaded once and cached, an
explicit path is loaded anew and leaves the cached instance alone, a missing library is a FileNotFoundError that says how to build it."""
import shutil

import pytest

import check_library as cl

# loader -> its key in api._LIBRARIES: libaesw.so, the host mirror, the build table's thirteen
LOADERS = dict({"load_library": "aesw", "load_host_library": "host"}, **{"load_%s_library" % n: n for n in cl.build_module().library_names()})


def test_every_library_of_the_loader_is_a_case(pkg):
    assert list(LOADERS.values()) == list(pkg.api._LIBRARIES) and len(LOADERS) == 15


@pytest.mark.parametrize("loader", LOADERS)
def test_default_is_cached_and_an_explicit_path_is_not(pkg, tmp_path, loader):
    load, (path, symbols, _hint) = getattr(pkg.api, loader), pkg.api._LIBRARIES[LOADERS[loader]]
    first = load()
    assert load() is first
    # a copy finds libaesw.so already mapped (its $ORIGIN no longer holds one): the loader maps that first
    copy = shutil.copy(path, tmp_path / path.name)
    other = load(copy)
    assert other is not first and load(copy) is not other
    assert load() is first
    assert all(getattr(other, name).restype is res for name, (res, _args) in symbols.items())  # the copy's symbols are bound as well


@pytest.mark.parametrize("loader", LOADERS)
def test_a_missing_library_says_how_to_build_it(pkg, tmp_path, loader):
    missing = tmp_path / "nowhere" / pkg.api._LIBRARIES[LOADERS[loader]][0].name
    with pytest.raises(FileNotFoundError) as e:
        getattr(pkg.api, loader)(missing)
    assert str(missing) in str(e.value) and "import __graft_entry__ as g; g.build()" in str(e.value)
    assert ("There is no fallback implementation." in str(e.value)) == (loader != "load_host_library")
