"""tests/development_forms.py held to itself and the oracle held to it, on the CPU: the tables against the reference's data files;
each piece of the form's algebra against a brute-force evaluation that does not use it; colorimetric anchors that hold whatever
the code does; the caps on what the assertions leave out, on the form alone; `oracle.film_develop` and
`oracle.film_develop_linear` against the form on every case; and the measurement the bounds come from."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import development_forms as df
import oracle
from pyrite_amd import project
from pyrite_amd.compiler import tables
from pyrite_amd.film import Film

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = [c.name for c in df.CASES]


# ------------------------------------------------------------------------------------------------ what both test files share
def expression(e):
    """A form's expression as the project module states it."""
    if e is None or isinstance(e, (int, float)):
        return e
    if e[0] == "curve":
        return project.spectrum(format="curve", points=[tuple(p) for p in e[1]])
    if e[0] == "array":
        return project.spectrum(format="array", min=e[1], max=e[2], points=list(e[3]))
    if e[0] == "blackbody":
        return project.blackbody(e[1])
    return {"d65": project.light_source.d65, "a": project.light_source.a}[e[0]]


def film_of(grains, span):
    height, width, bins, _ = grains.shape
    film = Film(width, height, bins, span)
    film.grains[...] = grains
    return film


def films_of(case):
    """(film, film_b or None, the keywords of develop / develop_linear / the oracle's entries)."""
    film = film_of(case.grains(), case.span)
    film_b = film_of(case.grains_b(), case.span) if case.halves else None
    return film, film_b, {"step_size": case.step, "filter": expression(case.filter), "white": expression(case.white)}


def check_linear(case, got, space, what, worst=None):
    """`got`: an XYZ or linear sRGB image of the case. Prints the figure, then asserts it against the class's bound."""
    form = case.form()
    key = {"xyz": "xyz", "srgb": "linear srgb"}[space]
    keep = ~form["left_out"]
    error = df.linear_error(got, form[{"xyz": "xyz", "srgb": "rgb"}[space]], form["scale"])[keep]
    figure = float(error.max()) if error.size else 0.0
    print("%s, %s, %s: largest |got - form| over the pixel's largest |XYZ| %.3g (bound %.3g), %d of %d pixels left out" % (case.name, what, key, figure, df.BOUNDS[key], (~keep).sum(), keep.size))
    if worst is not None:
        worst[key] = max(worst.get(key, 0.0), figure)
    assert np.isfinite(np.asarray(got)).all()
    assert figure <= df.BOUNDS[key], (case.name, what, key)
    assert (np.asarray(got).reshape(-1, 3)[-1] == 0).all(), "the last pixel is never developed (film.rs:299)"


def check_bytes(case, got, what):
    """`got`: the uint8 image of the case. A byte must be the form's; within the band around a rounding boundary, either."""
    form = case.form()
    keep = ~form["left_out"]
    wrong = df.wrong_bytes(got, form, df.BOUNDS["bytes"])[keep]
    print("%s, %s: %d of %d bytes wrong, %d in the rounding band, %d of %d pixels left out" % (case.name, what, wrong.sum(), wrong.size, df.in_band(form["e255"], df.BOUNDS["bytes"]).sum(), (~keep).sum(), keep.size))
    assert not wrong.any(), (case.name, what, np.argwhere(wrong)[:5].tolist())
    assert (np.asarray(got).reshape(-1, 3)[-1] == 0).all(), "the last pixel is never developed (film.rs:299)"


# ------------------------------------------------------------------------------------------------ 1. the tables
def nearest_f32(text):
    """The float32 nearest to a decimal numeral, checked in exact rationals: what a correctly rounding parser (Rust's f32::from_str,
    which the csv crate's serde support calls) makes of it -- not the double-rounded float(text) cast to f32."""
    exact, c = Fraction(text), np.float32(float(text))
    below, above = np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))
    assert abs(exact - Fraction(float(c))) < min(abs(exact - Fraction(float(below))), abs(exact - Fraction(float(above)))), text
    return c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def csv_tables():
    out = {}
    _, rows = df.read_csv("ciexyz65_1.csv")
    out["xyz"] = np.array([[nearest_f32(v) for v in r[1:4]] for r in rows], dtype=np.float32)
    out["xyz_w"] = [nearest_f32(r[0]) for r in rows]
    for name in ("d65", "a"):
        _, rows = df.read_csv(name + ".csv")
        out[name] = np.array([nearest_f32(r[1]) for r in rows], dtype=np.float32)
        out[name + "_w"] = [nearest_f32(r[0]) for r in rows]
    _, rows = df.read_csv("srgb_cie1931.csv")
    out["rgb_basis"] = np.array([[nearest_f32(v) for v in r] for r in rows], dtype=np.float32)
    return out


def test_the_csv_headers_are_the_ones_build_rs_deserializes():
    assert df.read_csv("ciexyz65_1.csv")[0] == ["wavelength", "x", "y", "z"]  # build.rs:123-129
    assert df.read_csv("d65.csv")[0] == df.read_csv("a.csv")[0] == ["wavelength", "intensity"]  # build.rs:189-193
    assert df.read_csv("srgb_cie1931.csv")[0] == ["r", "g", "b"]  # build.rs:61-66


def test_tables_npz_is_the_reference_data_bit_for_bit():
    want, got = csv_tables(), tables()
    assert sorted(got) == sorted(["xyz", "xyz_min", "xyz_max", "d65", "a", "light_min", "light_max", "rgb_basis", "rgb_min", "rgb_max"])
    assert got["xyz"].dtype == got["d65"].dtype == got["a"].dtype == got["rgb_basis"].dtype == np.float32
    assert got["xyz"].shape == (471, 3) and np.array_equal(bits(got["xyz"]), bits(want["xyz"]))
    assert got["d65"].shape == (107,) and np.array_equal(bits(got["d65"]), bits(want["d65"]))
    assert np.array_equal(bits(got["a"]), bits(want["a"] / np.float32(100.0)))  # build.rs:157, `intensity / 100.0` in f32
    assert got["rgb_basis"].shape == (471, 3) and np.array_equal(bits(got["rgb_basis"]), bits(want["rgb_basis"]))
    # the ranges as build.rs derives them: the extremes of the wavelength column (:85-86); one range over both lamp files (:145-146, :159-160); 360 + len (:37-38)
    assert (float(got["xyz_min"]), float(got["xyz_max"])) == (min(want["xyz_w"]), max(want["xyz_w"])) == (360.0, 830.0)
    assert (float(got["light_min"]), float(got["light_max"])) == (min(want["d65_w"] + want["a_w"]), max(want["d65_w"] + want["a_w"])) == (300.0, 830.0)
    assert (float(got["rgb_min"]), float(got["rgb_max"])) == (360.0, 360.0 + len(want["rgb_basis"])) == (360.0, 831.0)
    # Spectrum::Array assumes equal spacing: the files must have it, and one row per nanometre / per five
    assert want["xyz_w"] == list(range(360, 831)) and want["d65_w"] == want["a_w"] == list(range(300, 831, 5))


def test_the_forms_tables_are_the_same_numbers():
    got = tables()
    for name in ("xyz", "d65", "a", "rgb_basis"):
        assert np.array_equal(df.TABLES[name], got[name].astype(np.float64)), name
    for name in ("xyz_min", "xyz_max", "light_min", "light_max", "rgb_min", "rgb_max"):
        assert df.TABLES[name] == float(got[name]), name


def test_builtin_tables_inc_decodes_to_the_same_bits():
    text = open(os.path.join(ROOT, "pyrite_amd", "csrc", "host", "builtin_tables.inc")).read()
    got = tables()
    arrays = {m.group(1): (int(m.group(2)), m.group(3)) for m in re.finditer(r"static const uint32_t k_(\w+)_bits\[(\d+)\] = \{([^}]*)\};", text)}
    rows = {m.group(1): int(m.group(2)) for m in re.finditer(r"static const uint32_t k_(\w+)_rows = (\d+);", text)}
    floats = {m.group(1): m.group(2) for m in re.finditer(r"static const float k_(\w+) = ([-0-9.e+]+)f;", text)}
    assert sorted(arrays) == sorted(rows) == ["a", "d65", "rgb_basis", "xyz"]
    for name, (count, body) in arrays.items():
        words = np.array([int(w.strip().rstrip("u"), 16) for w in body.split(",")], dtype=np.uint32)
        assert count == len(words) == got[name].size and rows[name] == got[name].shape[0], name
        assert np.array_equal(words, bits(got[name]).reshape(-1)), name
    assert sorted(floats) == ["light_max", "light_min", "rgb_max", "rgb_min", "xyz_max", "xyz_min"]
    for name, literal in floats.items():
        assert np.float32(literal) == got[name], name


# ------------------------------------------------------------------------------------------------ 2. the form's algebra against brute force
SETTINGS = [((380.0, 780.0), 64, 2.0, None, None), ((380.0, 780.0), 64, 30.0, df.CURVE, df.WARM), ((380.0, 780.0), 255, 2.0, None, df.WARM),
            ((400.0, 700.0), 7, 2.0, df.CURVE, None), ((500.0, 510.0), 4, 30.0, None, None), ((500.0, 516.0), 16, 0.5, None, df.WARM), ((400.0, 701.0), 5, 2.0, None, None)]


@pytest.mark.parametrize("span,bins,step,filter,white", SETTINGS)
def test_the_linear_map_is_the_sample_by_sample_walk(span, bins, step, filter, white):
    rng = np.random.default_rng(1)
    a = df.linear_map(span, bins, step, filter, white)
    for _ in range(3):
        q = rng.normal(size=bins)
        want = df.walk(q, span, step, filter, white)
        assert np.abs(a @ q - want).max() <= 1e-12 * np.abs(a).sum(axis=1).max() * np.abs(q).max()
    for b in (0, bins // 2, bins - 1):  # and column by column
        assert np.allclose(a[:, b], df.walk(np.eye(bins)[b], span, step, filter, white), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("span,bins,step,filter,white", SETTINGS)
def test_the_walk_is_numpys_trapezoid_over_the_samples(span, bins, step, filter, white):
    q = np.random.default_rng(2).uniform(0.1, 1.0, size=bins)
    w = np.array([float(x) for x in df.sample_points(span, step)])
    assert w[0] == span[0] and w[-2] < span[1] <= w[-1] and np.all(np.diff(w) == step)
    inside = (w >= span[0]) & (w <= span[1])
    index = np.minimum(np.floor((w - span[0]) / (span[1] - span[0]) * bins + 1e-9), bins - 1).astype(int)  # float floor, nudged over the edges
    value = np.where(inside, q[np.clip(index, 0, bins - 1)], 0.0) * df.gains(span, step, filter, white)
    response = np.array([df.observer(x) for x in w])
    want = np.array([np.trapezoid(value * response[:, c], w) for c in range(3)]) / (len(w) - 1) / step * 3.444
    assert np.allclose(df.walk(q, span, step, filter, white), want, rtol=1e-12, atol=1e-15)


def test_step_30_weighs_420_nm():
    w = df.sample_points((380.0, 780.0), 30.0)
    assert len(w) == 15 and w[-2:] == [770, 800]  # main.rs:397: the last step starts below max and ends beyond it
    flat = df.walk(np.ones(64), (380.0, 780.0), 30.0)
    inner = np.array([df.observer(380.0 + 30.0 * k) for k in range(14)])  # the sample at 800 sees no film
    assert np.allclose(flat, (inner.sum(axis=0) - 0.5 * inner[0]) * 30.0 / 420.0 * 3.444, rtol=1e-13)


def test_bins_edges_and_the_ends_of_the_span():
    span = (380.0, 780.0)
    assert df.bin_of(span, 64, 380.0) == 0 and df.bin_of(span, 64, 780.0) == 63  # w == max: the last bin, not 0 and not bin 64
    assert df.bin_of(span, 64, 379.99) is None and df.bin_of(span, 64, 780.01) is None
    assert df.bin_of(span, 64, 430.0) == 8 and df.bin_of(span, 64, 429.99) == 7  # an edge belongs to the upper bin
    assert df.bin_of(span, 3, 646.0) == 1 and df.bin_of(span, 3, 648.0) == 2  # floor, not round: 646 is 1.995 bins in
    with pytest.raises(ValueError):
        df.sample_points((380.0, 780.0), 0.1)  # 0.1 is no f32 number
    with pytest.raises(ValueError):
        df.sample_points((380.1, 780.0), 2.0)
    assert df.uncertain_edges(span, 64, 2.0) == [] and df.uncertain_edges(span, 64, 30.0) == []
    assert df.uncertain_edges(span, 255, 2.0) == [(50, 51), (101, 102), (152, 153), (203, 204)]  # fifths of the span
    assert len(df.uncertain_edges(span, 5, 2.0)) == 4 and df.uncertain_edges((400.0, 701.0), 5, 2.0) == []


def test_lookups_keep_their_ends():
    t = df.TABLES
    assert np.array_equal(df.observer(300.0), t["xyz"][0]) and np.array_equal(df.observer(900.0), t["xyz"][-1])  # end values, not zero
    assert np.allclose(df.observer(555.5), 0.5 * (t["xyz"][195] + t["xyz"][196]), rtol=1e-13)
    assert df.curve_get(df.CURVE[1], 450.0) == 0.0 and df.curve_get(df.CURVE[1], 651.0) == 0.0 and df.curve_get(df.CURVE[1], 700.0) == 0.0
    assert df.curve_get(df.CURVE[1], 455.5) == 0.25 and df.curve_get(df.CURVE[1], 550.0) == 0.875
    assert df.evaluate(("array", 400.0, 700.0, [1.0, 3.0, 2.0]), 350.0) == 1.0 and df.evaluate(("array", 400.0, 700.0, [1.0, 3.0, 2.0]), 625.0) == 2.5
    # Wien's displacement law: the 4000 K curve peaks at 2.8978e6 / 4000 = 724.4 nm
    w = np.arange(600.0, 900.0, 0.5)
    assert abs(w[np.argmax([df.blackbody(x, 4000.0) for x in w])] - 724.4) <= 0.5


def test_quotients():
    g = np.array([[[2.0, 4.0], [1.0, 0.0], [3.0, -1.0], [-1.0, 2.0]]], dtype=np.float32)
    assert df.quotients(g).tolist() == [[0.5, 0.0, 0.0, -0.5]]  # weight <= 0: 0 (film.rs:138-142)
    h = np.array([[[1.0, 2.0], [1.0, 0.5], [3.0, 1.0], [0.0, 0.0]]], dtype=np.float32)
    assert df.quotients(g, h).tolist() == [[0.5, 4.0, 0.0, -0.5]]  # (accA + accB) / (wA + wB)


def test_the_matrix_meets_its_conditions():
    m = df.xyz_to_rgb_matrix()
    for k, (x, y) in enumerate(df.PRIMARIES):  # a primary's chromaticity maps to a multiple of its unit vector ...
        rgb = m @ np.array([x / y, 1.0, (1.0 - x - y) / y])
        assert np.abs(rgb / rgb[k] - np.eye(3)[k]).max() <= 1e-13
    assert np.abs(m @ np.array(df.WHITE_POINT) - 1.0).max() <= 1e-13  # ... scaled so that the white point maps to (1, 1, 1)
    forward = np.linalg.inv(m)
    assert np.abs(forward.sum(axis=1) - np.array(df.WHITE_POINT)).max() <= 1e-13 and np.abs(forward[1].sum() - 1.0) <= 1e-13
    literals = np.array([[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]])  # main.hip, film.hip, tone.hip, oracle.cpp
    print("largest |derived - literal| of the matrix: %.3g" % np.abs(m - literals).max())
    assert np.abs(m - literals).max() <= 5e-8


def test_the_encoding():
    assert np.abs(df.encode255([-1.0, 0.0, 2.0]) - [0.0, 0.0, 255.0]).max() <= 1e-12  # clamped first
    assert abs(df.encode255(0.0031308) - 255 * 12.92 * 0.0031308) < 1e-12 and abs(df.encode255(0.0031309) - 255 * 12.92 * 0.0031309) < 1e-4  # the pieces meet
    assert np.floor(df.encode255([0.5, 0.18, 0.001]) + 0.5).tolist() == [188.0, 118.0, 3.0]  # IEC 61966-2-1: 0.5 -> 0.7354, 0.18 -> 0.4614, 0.001 -> 0.01292


# ------------------------------------------------------------------------------------------------ 3. colorimetric anchors
def integrate(values, w):
    return np.trapezoid(values, w, axis=0)


def test_the_observer_and_d65_data():
    t = df.TABLES
    w = np.arange(360.0, 831.0)
    x, y, z = integrate(t["xyz"], w)
    print("observer integrals over 360-830: %.3f %.3f %.3f" % (x, y, z))
    assert max(x, y, z) / min(x, y, z) - 1.0 <= 3e-4  # an equal-energy spectrum is white: the three integrals agree within 0.03 %
    assert np.allclose([x, y, z], [116.649, 116.662, 116.674], atol=1e-3)
    assert abs(t["xyz"][:, 1].max() - 1.0) <= 1e-3  # y-bar peaks at 1
    assert 360 + int(np.argmax(t["xyz"][:, 1])) == 557  # at 557 nm: with the three integrals above, the table is the CIE 1964 10-degree observer (1931's peaks at 555)
    assert df.d65(560.0) == 1.0  # the file is D65 normalised at 560 nm


def d65_xyz_direct():
    """X, Y, Z of D65 over 380-780 straight from the two files: a 1 nm trapezoid, normalised by nothing."""
    w = np.arange(380.0, 781.0)
    lamp = np.interp(w, np.arange(300.0, 831.0, 5.0), df.TABLES["d65"])
    return integrate(df.TABLES["xyz"][20:421] * lamp[:, None], w)


def test_a_d65_film_develops_to_the_chromaticity_of_the_data():
    """400 bins of 1 nm, each holding D65 at its centre; developed at step 1 every inner sample sits on an edge (quotient k/400: the
    form REFUSES nothing, the f32 code might differ, which is why this anchor is the form's alone) and reads the bin above."""
    span, bins = (380.0, 780.0), 400
    centre = 380.5 + np.arange(bins)
    q = np.array([df.d65(x) for x in centre])
    xyz = df.linear_map(span, bins, 1.0) @ q
    # exactly: the sample at 380 + k reads the bin above it, D65 at 380.5 + k (the one at 780 the last bin, 779.5)
    w = np.arange(380.0, 781.0)
    shifted = np.array([df.d65(min(x + 0.5, 779.5)) for x in w])
    assert np.allclose(xyz, 3.444 / 400.0 * integrate(df.TABLES["xyz"][20:421] * shifted[:, None], w), rtol=1e-12)
    direct = d65_xyz_direct()
    # against the data itself the film is half a nanometre late. D65 moves by at most 2 % per nanometre (0.1 of its value between
    # two 5 nm rows), so no tristimulus value moves by more than 1 %; the chromaticity differs by 5.7e-4 at most
    print("chromaticity of the D65 film - of the data: %s" % (xyz / xyz.sum() - direct / direct.sum()))
    assert np.abs(xyz / xyz.sum() - direct / direct.sum()).max() <= 1e-3
    rgb = df.xyz_to_rgb_matrix() @ (direct / direct[1])
    print("D65 over 380-780 through the matrix, Y = 1: linear sRGB %.4f %.4f %.4f" % tuple(rgb))
    assert np.allclose(rgb, [1.0002, 1.0016, 0.9832], atol=2e-4)  # the data's own D65 is this far from the matrix's white point: blue 1.7 % short
    # and the absolute level: 3.444 / 400 * integral(observer D65) -- what an albedo-1 floor under D65 develops to
    level = 3.444 / 400.0 * direct
    print("an albedo-1 D65 film develops to XYZ %.4f %.4f %.4f, linear sRGB %.4f %.4f %.4f" % (tuple(level) + tuple(df.xyz_to_rgb_matrix() @ level)))
    assert np.allclose(df.xyz_to_rgb_matrix() @ level, [1.0007, 1.0021, 0.9837], atol=2e-4)
    assert np.allclose(xyz, level, rtol=1e-2)  # half a nanometre of D65's slope, as above


def test_a_balanced_blackbody_film_has_the_d65_films_colour():
    """A fine-binned film of blackbody(4000), balanced with white = blackbody(4000), develops to a multiple of the D65 film's colour:
    s / (white / max_white) * D65 / max_d65 turns the one spectrum into the other (main.rs:216-221)."""
    span, bins = (380.0, 780.0), 400
    centre = 380.5 + np.arange(bins)
    warm = np.array([df.blackbody(x, 4000.0) for x in centre])
    balanced = df.linear_map(span, bins, 1.0, white=df.WARM) @ warm
    plain = df.linear_map(span, bins, 1.0) @ np.array([df.d65(x) for x in centre])
    ratio = balanced / plain
    assert np.abs(ratio / ratio.mean() - 1.0).max() <= 1e-3  # bins of 1 nm against samples on their edges: half a nanometre of slope
    most, most_d65 = df.white_maxima(span, df.WARM)
    assert most == df.blackbody(724.0, 4000.0) and most_d65 == max(df.d65(float(x)) for x in range(380, 780))  # the 1 nm scan, below max
    # the level: the film holds the curve half a nanometre above each sample, and Planck's curve at 4000 K rises by at most
    # -5 / w + 1.4388e7 / (w^2 T) = 1.2 % per nanometre (at 380 nm): within 0.6 %
    assert abs(ratio.mean() - most / most_d65) <= 6e-3 * most / most_d65
    raw = df.linear_map(span, bins, 1.0) @ warm  # unbalanced, 4000 K is reddish: more X than Z by far
    assert raw[0] / raw[2] > 1.5 * plain[0] / plain[2]


# ------------------------------------------------------------------------------------------------ 4. the caps, on the form alone
@pytest.mark.parametrize("case", df.CASES, ids=CASE_IDS)
def test_caps_on_what_is_left_out(case):
    form = case.form()
    pixels = len(form["q"])
    left, band = form["left_out"][:-1], df.in_band(form["e255"][:-1], df.BOUNDS["bytes"])
    print("%s: %d of %d pixels left out, %d of %d bytes in the rounding band" % (case.name, left.sum(), pixels, band.sum(), band.size))
    assert np.isfinite(df.BOUNDS["bytes"]) and df.BOUNDS["bytes"] < 0.25
    if pixels > 1:
        assert left.mean() <= df.MOST_LEFT_OUT and band.mean() <= df.MOST_IN_BAND
    if case.span == df.DEFAULT_SPAN and case.grains().shape[2] == 64:
        assert not left.any()  # every edge sample is an eighth of the span: exact
    assert form["scale"].max() <= 8.0  # the byte band is absolute: the films stay in the range where f32 resolves it
    if pixels > 1:
        assert len(np.unique(form["bytes"][:-1], axis=0)) >= min(pixels - 1, 8) // 2, "a picture of one colour shows nothing"


def test_the_cases_are_the_ones_the_kernels_need():
    bins = sorted({c.grains().shape[2] for c in df.CASES if c.name.startswith("one hot") and c.span == df.DEFAULT_SPAN})
    assert bins == [1, 2, 3, 64, 127, 128, 129, 255, 256]
    for c in df.CASES:
        g = c.grains()
        if c.name.startswith("one hot"):
            assert g.shape[0] * g.shape[1] == max(130, 2 * g.shape[2] + 3)
            q = df.quotients(g)[0]
            assert ((q != 0).sum(axis=1) == 1).all() and (np.argmax(q != 0, axis=1) == np.arange(len(q)) % g.shape[2]).all()
        if c.name.startswith("random"):
            q = df.quotients(g)
            assert g.shape[0] * g.shape[1] == 1 or ((g[..., 1] == 0).mean() > 0.05 and (q < 0).any())
    assert [c.grains().shape[:3] for c in df.CASES if c.name.startswith("long")] == [(64, 8193, 1), (64, 16385, 1)]
    assert 8193 > df.WAVE_GRID and 16385 * 64 > df.PIXEL_GRID  # a second trip of the run loop; of the grid stride


# ------------------------------------------------------------------------------------------------ 5. the oracle against the form
WORST = {}


def oracle_e255_figure(case):
    film, _, settings = films_of(case)
    form = case.form()
    e255 = oracle.film_develop_linear(film, "encoded", **settings).reshape(-1, 3)
    return float(np.abs(e255.astype(np.float64) - form["e255"])[~form["left_out"]].max(initial=0.0))


@pytest.mark.parametrize("case", df.CASES, ids=CASE_IDS)
def test_the_oracle_develops_what_the_form_states(case):
    film, film_b, settings = films_of(case)
    for space in ("xyz", "srgb"):
        check_linear(case, oracle.film_develop_linear(film, space, film_b, **settings), space, "oracle", WORST)
    if not case.halves:
        figure = oracle_e255_figure(case)
        print("%s, oracle: largest |255 e - form's| %.3g bytes (band %.3g)" % (case.name, figure, df.BOUNDS["bytes"]))
        WORST["bytes"] = max(WORST.get("bytes", 0.0), figure)
        assert figure <= df.BOUNDS["bytes"]
        check_bytes(case, oracle.film_develop(film, **settings), "oracle")


def test_measured_figures_are_the_ones_the_bounds_come_from():
    """MEASURED is the largest |oracle - form| of each class over every case, to two digits: measured here again, and written to
    the file PYRITE_DEVELOPMENT_FORMS_REPORT names (profiles/r26_development_forms.txt keeps a run; nothing reads it back)."""
    worst, lines = {}, []
    for case in df.CASES:
        film, film_b, settings = films_of(case)
        form = case.form()
        figures = {}
        for space, key, field in (("xyz", "xyz", "xyz"), ("srgb", "linear srgb", "rgb")):
            got = oracle.film_develop_linear(film, space, film_b, **settings)
            figures[key] = float(df.linear_error(got, form[field], form["scale"])[~form["left_out"]].max(initial=0.0))
        if not case.halves:
            figures["bytes"] = oracle_e255_figure(case)
        for key, figure in figures.items():
            worst[key] = max(worst.get(key, 0.0), figure)
        lines.append("%-52s xyz %.3g  linear srgb %.3g  bytes %s  left out %d of %d  in band %d of %d" % (
            case.name, figures["xyz"], figures["linear srgb"], "%.3g" % figures["bytes"] if "bytes" in figures else "-", form["left_out"].sum(), len(form["q"]),
            df.in_band(form["e255"], df.BOUNDS["bytes"]).sum(), form["e255"].size))
    print("\n".join(lines))
    print("worst:", worst)
    report = os.environ.get("PYRITE_DEVELOPMENT_FORMS_REPORT")
    if report:
        with open(report, "w") as f:
            f.write("largest |oracle - form| per case, CPU: xyz and linear srgb over the pixel's largest |XYZ|, bytes as |255 e - form's 255 e|\n")
            f.write("\n".join(lines) + "\n")
            f.write("worst: %s\nMEASURED: %s\nBOUNDS (4 x MEASURED): %s\n" % (worst, df.MEASURED, df.BOUNDS))
    for key, figure in worst.items():
        assert df.MEASURED[key] is not None, "measure first: %s" % worst
        assert figure <= df.MEASURED[key] <= 1.25 * figure, (key, figure, df.MEASURED[key])
