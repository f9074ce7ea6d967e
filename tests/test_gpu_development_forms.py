"""Film development on the GPU against tests/development_forms.py, the float64 form that imports neither the product nor the oracle:
`develop` under both of its kernels (PYRITE_DEVELOP_KERNEL=pixel: develop_kernel, =wave: develop_wave_kernel), `develop_linear` in
XYZ and in linear sRGB (develop_linear_kernel up to 255 bins, develop_linear_pixel_kernel beyond), and the two-half form. The
assertions, the cases and the constants are the ones tests/test_development_forms_cpu.py holds the oracle to; the bounds were
measured there, on the CPU."""
import numpy as np
import pytest

import development_forms as df
from pyrite_amd.develop import develop, develop_linear
from test_development_forms_cpu import check_bytes, check_linear, films_of

pytestmark = pytest.mark.gpu

BYTE_RUNS = [(c, form) for c in df.CASES if not c.halves for form in c.forms]  # 256 bins: the wave form's rows do not hold them


@pytest.mark.parametrize("case,form", BYTE_RUNS, ids=["%s, %s" % (c.name, form) for c, form in BYTE_RUNS])
def test_develop_gives_the_forms_bytes(case, form, gpu_lib, monkeypatch):
    monkeypatch.setenv("PYRITE_DEVELOP_KERNEL", form)  # read at every call
    film, _, settings = films_of(case)
    got = develop(film, **settings)
    assert got.shape == (film.height, film.width, 3) and got.dtype == np.uint8
    check_bytes(case, got, "develop, " + form)


@pytest.mark.parametrize("space", ["xyz", "srgb"])
@pytest.mark.parametrize("case", df.CASES, ids=[c.name for c in df.CASES])
def test_develop_linear_gives_the_forms_values(case, space, gpu_lib):
    film, film_b, settings = films_of(case)
    got = develop_linear(film, space, film_b, **settings)
    assert got.shape == (film.height, film.width, 3) and got.dtype == np.float32
    check_linear(case, got, space, "develop_linear" + (", two halves" if film_b is not None else ""))
