"""Powder characterisation (ampis/applications/powder.py): satellites matched to their particles, the satellite content of a sample and the
particle size distribution -- the reference's names, arguments, result keys and printed lines, laid out for the C ABI instead of for pycocotools:

  * The reference builds RLE.merge([satellite, particle], intersect=True) and takes RLE.area for EVERY satellite against EVERY particle of an
    image in a Python loop (:80-83; 30 000 - 40 000 merges a micrograph), once per image of a sample.  Here ONE amp_rle_overlap_groups call
    returns the exact pixel count of every pair of every image (group = image), on the device (csrc/rle_overlap.hip) or on the host; a single
    micrograph is too little work for a card, the sample is the unit of a launch.
  * The matching rule as array semantics: satellite s has the score float64(|s AND p|) / float64(|s|) with every particle p of its image; it
    takes the particle of maximal score, the FIRST among equals (lowest index), and is matched iff that score is strictly greater than
    `match_thresh`.  A particle may take several satellites; a satellite takes one particle.
  * Three stated departures, where the reference raises or warns: no match at all gives an empty [0, 2] array and {} (the reference: IndexError
    at :101); no particles leave every satellite unmatched (the reference: ValueError from argmax of nothing); a satellite without a pixel is
    unmatched, without the 0 / 0 warning.

An "instance set" is duck-typed like analyze.compute_rprops: anything with .instances.masks, .instances.image_size, .HFW and .HFW_units.
`visualize_particle_with_satellites` is plotting and is not part of this module."""
import copy
import numbers

import numpy as np

from .. import analyze, rle


def _to_rle(x, size=None):
    """RLE list of an instance set, an Instances-like object (.masks, .image_size) or anything analyze.masks_to_rle accepts."""
    if hasattr(x, "instances"):
        x = x.instances
    if hasattr(x, "masks") and not hasattr(x, "rle"):
        if size is None and hasattr(x, "image_size"):
            size = tuple(int(v) for v in x.image_size)
        x = x.masks
    return analyze.masks_to_rle(x, size)


def _match_from_overlap(inter, area_sat, n_particles, match_thresh):
    """The rule of the module docstring on inter [n_satellites, n_particles] (pixels in both) and area_sat [n_satellites] -> the result dict."""
    ns = len(area_sat)
    hit, taken, best = np.zeros(ns, bool), np.zeros(ns, np.int64), np.zeros(ns, np.float64)
    if ns and n_particles:
        valid = area_sat > 0                                        # a satellite without a pixel scores 0 / 0: unmatched
        score = np.zeros((ns, n_particles), np.float64)
        score[valid] = inter[valid].astype(np.float64) / area_sat[valid].astype(np.float64)[:, None]
        taken = score.argmax(axis=1)                                # first maximum of each row
        best = score[np.arange(ns), taken]
        hit = valid & (best > match_thresh)                         # strict
    matched = np.zeros(n_particles, bool)
    matched[taken[hit]] = True
    sat_idx, par_idx = np.flatnonzero(hit), taken[hit]
    match_pairs = {int(p): [] for p in np.flatnonzero(matched)}
    for s, p in zip(sat_idx.tolist(), par_idx.tolist()):
        match_pairs[p].append(s)
    return {"satellite_matches": np.stack([sat_idx, par_idx], axis=1).astype(np.int64).reshape(-1, 2), "satellites_unmatched": np.flatnonzero(~hit),
            "particles_unmatched": np.flatnonzero(~matched), "intersection_scores": best[hit], "match_pairs": match_pairs}


def satellite_match_many(pairs, match_thresh=0.5, device='auto'):
    """satellite_match for a list of (particles, satellites), one entry per image -> the list of result dicts.  ALL images go through one
    amp_rle_overlap_groups call (group = image).  ValueError for a bad `device` and for an image whose masks differ in size."""
    groups = [(_to_rle(p), _to_rle(s)) for p, s in pairs]
    ctx = analyze._device_context("satellite_match_many", device, any(len(p) and len(s) for p, s in groups))
    inters, areas_s, _ = rle.overlap_groups([s for _, s in groups], [p for p, _ in groups], ctx=ctx)
    return [_match_from_overlap(i, a, len(p), match_thresh) for i, a, (p, _) in zip(inters, areas_s, groups)]


def satellite_match(particles, satellites, match_thresh=0.5, device='auto', size=None):
    """Match the satellites of an image to its particles (ampis/applications/powder.py:28-112, same result keys).

    particles, satellites: instance sets, Instances-like objects or anything analyze.masks_to_rle accepts (size=(h, w) for bare polygon masks);
    match_thresh: a satellite matches iff its best score is strictly above it; device: 'cpu' (host), 'cuda' (HIP device, an error without
    one) or 'auto' (the device when one is visible) -- identical results.  Returns
      'satellite_matches'     [n_match, 2] int64 (satellite index, particle index), in satellite order;
      'satellites_unmatched'  indices of the satellites without a particle;
      'particles_unmatched'   indices of the particles without a satellite;
      'intersection_scores'   [n_match] float64, |satellite AND particle| / |satellite| of each match;
      'match_pairs'           {particle index: [satellite indices in satellite order]}, particles in ascending order.
    The rule and the three departures from the reference are in the module docstring."""
    ps, ss = _to_rle(particles, size), _to_rle(satellites, size)
    ctx = analyze._device_context("satellite_match", device, len(ps) and len(ss))
    try:
        inters, areas_s, _ = rle.overlap_groups([ss], [ps], ctx=ctx)
    except ValueError as e:
        raise ValueError(str(e).replace("overlap_groups: group 0 holds", "satellite_match: particles / satellites hold")) from None
    return _match_from_overlap(inters[0], areas_s[0], len(ps), match_thresh)


_rle_satellite_match = satellite_match          # the reference's name


class PowderSatelliteImage(object):
    """Powder and satellite instance predictions for a single image (ampis/applications/powder.py:115): `particles` and `satellites` are
    instance sets, `matches` a satellite_match result or None."""

    def __init__(self, particles=None, satellites=None, matches=None):
        self.particles = particles
        self.satellites = satellites
        self.matches = matches

    def compute_matches(self, thresh=0.5, device='auto'):
        """Stores satellite_match(self.particles, self.satellites, thresh) in self.matches."""
        self.matches = satellite_match(self.particles, self.satellites, thresh, device=device)

    def compute_satellite_metrics(self):
        """{'n_satellites', 'n_particles_matched', 'n_particles_all', 'mask_areas_matched', 'mask_areas_all'}: the counts of the image and the
        particle mask areas (all, and those with at least one satellite), so that a size filter can be applied before counting."""
        assert self.particles is not None and self.satellites is not None and self.matches is not None
        matched_particle_idx = np.asarray(list(self.matches["match_pairs"]), dtype=np.int64)
        mask_areas_all = rle.area(_to_rle(self.particles))
        return {"n_satellites": len(_to_rle(self.satellites)), "n_particles_matched": len(matched_particle_idx),
                "n_particles_all": len(mask_areas_all), "mask_areas_matched": mask_areas_all[matched_particle_idx], "mask_areas_all": mask_areas_all}

    def copy(self):
        return copy.deepcopy(self)


def _is_psi(x):
    return hasattr(x, "particles") and hasattr(x, "satellites") and hasattr(x, "matches")


def psd(particles, xvals='d_eq', yvals='cvf', c=None, distance='length', ax=None, plot=True, return_results=False):
    """Cumulative particle size distribution from segmentation masks (ampis/applications/powder.py:288-461: same arguments, same result keys).

    particles: an instance set or PowderSatelliteImage, a list of them, or a list of arrays of mask areas in pixels (one per image);
    xvals: 'd_eq' (equivalent circle diameter 2 sqrt(A / pi)) or 'area'; yvals: 'cvf' (cumulative volume fraction) or 'counts' (cumulative
    fraction of the instances); c: length of one pixel -- any real number for all images, a list / array with one value per image, a tuple
    (value or list, units) or None (HFW / image width of every instance set); distance: 'length' (apply c) or 'pixels'; ax / plot: where and
    whether to draw (matplotlib is imported only then); return_results: return {'x', 'y', 'x_label', 'y_label'}.

    The values are the reference's, also where it departs from its own docstring: the 'cvf' weight of a bin is 4/3 pi^(-1/2) u^(3/2) of the
    bin's x value u AFTER the conversion -- with xvals='d_eq' of the diameters, not of the areas -- which is what existing plots show.
    Unlike the reference: arrays of areas work (it fails on them), c may be any real number, and nothing but the result is printed.
    ValueError for unknown xvals / yvals / distance, a c of another type, and distance='length' without c on particles that carry no HFW."""
    if isinstance(c, tuple):
        length_units, c = c[1], c[0]
    else:
        length_units = ''
    if _is_psi(particles) or hasattr(particles, "instances"):
        particles = [particles]
    particles = [x.particles if _is_psi(x) else x for x in particles]
    isets = all(hasattr(x, "instances") for x in particles)
    areas = [np.asarray(analyze.mask_areas(x)) if hasattr(x, "instances") else np.asarray(x) for x in particles]

    if distance.lower() == 'length':
        if c is None:
            if not (len(particles) and isets):
                raise ValueError('Cannot infer c from particles (must be list of InstanceSet or PowderSatelliteImage objects')
            if particles[0].HFW is None:
                raise ValueError('Cannot infer c because HFW is not defined')
            assert all(x.HFW is not None for x in particles), 'all HFW values must be specified if c is not defined'
            for iset in particles:
                assert iset.HFW_units == particles[0].HFW_units, 'all HFW values should have same units'
            length_units = particles[0].HFW_units
            c = [x.HFW / int(x.instances.image_size[1]) for x in particles]       # horizontal field width / width in pixels
        if isinstance(c, (list, np.ndarray)):
            assert len(c) == len(areas), 'if c (or c[0] if passed as tuple) is a list or array it must have the same length as particles.'
            areas = [a_i.astype(np.float64) * float(c_i) ** 2 for a_i, c_i in zip(areas, c)]
        elif isinstance(c, numbers.Real):
            areas = [a_i.astype(np.float64) * float(c) ** 2 for a_i in areas]
        else:
            raise ValueError('c (or c[0] if passed as tuple) must be a list, array, int, or float')
    elif distance.lower() == 'pixels':
        length_units = 'px'
    else:
        raise ValueError('distance must be "length" or "pixels"')

    areas = np.concatenate(areas, axis=0) if len(areas) else np.zeros(0)
    unique, counts = np.unique(areas, return_counts=True)
    if xvals.lower() == 'd_eq':
        unique = 2 * np.sqrt(unique / np.pi)
        xlabel = 'Equivalent diameter{}'.format(', {}'.format(length_units) if length_units else '')
    elif xvals.lower() == 'area':
        xlabel = 'Mask area{}'.format('- ${}^2$'.format(length_units) if length_units else '')
    else:
        raise ValueError('xvals must be "d_eq" or "area"')

    if yvals.lower() == 'cvf':
        volumes = 4 / 3 * np.pi ** (-1 / 2) * unique ** (3 / 2)      # of the converted x values: see the docstring
        counts = volumes * counts
        ylabel = 'cumulative volume fraction'
    elif yvals.lower() == 'counts':
        ylabel = 'counts (cumulative)'
    else:
        raise ValueError('yvals must be "cvf" or "counts"')
    counts = counts.cumsum()
    counts = counts / counts[-1] if len(counts) else counts.astype(np.float64)
    x, y = unique, counts

    if plot or ax is not None:
        import matplotlib.pyplot as plt
        if ax is None:
            fig, ax = plt.subplots(dpi=300)
        ax.grid(axis='both', which='both', color=(0.85, 0.85, 0.85), linewidth=1, linestyle='--')
        ax.plot(x, y, '-.k')
        ax.set_xlabel(xlabel)
        ax.set_ylabel(ylabel)
        if plot:
            plt.show()
    if return_results:
        return {'x': x, 'y': y, 'x_label': xlabel, 'y_label': ylabel}


def satellite_measurements(psi, print_summary=True, output_dict=False, device='auto'):
    """The satellite content of the sample `psi`, a PowderSatelliteImage or a list of them (ampis/applications/powder.py:463-569: same keys,
    labels and printed lines).  When any psi[i].matches is None, the matches of ALL images are computed with the default threshold in one
    satellite_match_many call and stored.  Keys of the dict (returned when output_dict): n_images, n_particles, n_satellites (matched),
    n_satellites_unmatched, n_satellited_particels (sic), sat_frac, mspp (median satellites per satellited particle),
    unique_satellites_per_particle, counts_satellites_per_particle (cumulative, relative).  A sample without a match has mspp = nan, one
    without a particle sat_frac = nan (the reference warns / divides by zero there)."""
    if _is_psi(psi):
        psi = [psi]
    assert all(_is_psi(x) for x in psi), 'psi must be list of PowderSatelliteImage objects!'
    if any(x.matches is None for x in psi):
        for x, m in zip(psi, satellite_match_many([(x.particles, x.satellites) for x in psi], device=device)):
            x.matches = m
    matches = [x.matches for x in psi]

    n_images = len(psi)
    n_particles_matched = sum(len(x['match_pairs']) for x in matches)
    n_particles = n_particles_matched + sum(len(x['particles_unmatched']) for x in matches)
    spp_list = np.asarray([len(v) for m in matches for v in m['match_pairs'].values()], dtype=np.int64)      # satellites per particle
    n_satellites_matched = int(spp_list.sum())
    mspp = np.median(spp_list) if len(spp_list) else float('nan')
    n_satellites_unmatched = sum(len(x['satellites_unmatched']) for x in matches)
    sat_frac = n_particles_matched / n_particles if n_particles else float('nan')

    unique, counts = np.unique(spp_list, return_counts=True)
    assert counts.sum() == n_particles_matched
    assert n_particles == sum(len(_to_rle(x.particles)) for x in psi)
    assert n_satellites_matched + n_satellites_unmatched == sum(len(_to_rle(x.satellites)) for x in psi)
    counts = counts.cumsum() / counts.sum() if len(counts) else counts.astype(np.float64)

    keys = ['n_images', 'n_particles', 'n_satellites', 'n_satellites_unmatched', 'n_satellited_particels',
            'sat_frac', 'mspp', 'unique_satellites_per_particle', 'counts_satellites_per_particle']
    labels = ['number of images',
              'number of particles',
              'number of matched satellites',
              'number of unmatched satellites',
              'number of satellited particles',
              'fraction of satellited particles',
              'median number of satellites per\n'
              'satellited particle             ']
    values = [n_images, n_particles, n_satellites_matched, n_satellites_unmatched, n_particles_matched, sat_frac, mspp, unique, counts]
    if print_summary:
        for lab, v in zip(labels, values[:-2]):
            print('{:35}\t{}'.format(lab, v))
    if output_dict:
        return dict(zip(keys, values))
