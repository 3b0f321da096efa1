"""A minimal FITS reader for the star tool (helios_amd/star.py): astropy where it is installed, this module otherwise, as
hdf5_lite stands in for h5py.

What it reads: header blocks of 2880 bytes (80-character cards up to END), a primary image of BITPIX -32, -64, 16 or 32 with
one or two axes, and BINTABLE extensions whose columns are scalar numbers (`E`, `D`, `J`, `K`).  FITS data are big-endian;
arrays come back in the machine's byte order with the file's values bit for bit.  BSCALE / BZERO other than 1 / 0 are applied
as astropy applies them (the result is floating point then).
"""
import numpy as np

BLOCK = 2880
_IMAGE = {-32: ">f4", -64: ">f8", 16: ">i2", 32: ">i4"}
_COLUMN = {"E": ">f4", "D": ">f8", "J": ">i4", "K": ">i8"}


def _value(text):
    text = text.split("/")[0].strip() if not text.strip().startswith("'") else text.strip()
    if text.startswith("'"):
        return text[1:text.index("'", 1)].rstrip()
    if text in ("T", "F"):
        return text == "T"
    try:
        return int(text)
    except ValueError:
        try:
            return float(text.replace("D", "E"))
        except ValueError:
            return text


def _read_header(f, path):
    cards = {}
    while True:
        block = f.read(BLOCK)
        if len(block) < BLOCK:
            raise IOError("fits_lite: %s ends inside a header" % path)
        for k in range(0, BLOCK, 80):
            card = block[k:k + 80].decode("ascii", "replace")
            key = card[:8].strip()
            if key == "END":
                return cards
            if card[8:10] == "= ":
                cards[key] = _value(card[10:])


def _data_bytes(h):
    naxis = int(h.get("NAXIS", 0))
    if naxis == 0:
        return 0
    n = abs(int(h["BITPIX"])) // 8
    for k in range(1, naxis + 1):
        n *= int(h["NAXIS%d" % k])
    return n + int(h.get("PCOUNT", 0))


def _image(h, raw, path):
    bitpix, naxis = int(h["BITPIX"]), int(h.get("NAXIS", 0))
    if bitpix not in _IMAGE or naxis not in (1, 2):
        raise IOError("fits_lite: %s holds an image of BITPIX %d with %d axes; BITPIX -32, -64, 16 or 32 with one or two axes "
                      "are read (install astropy for the rest)" % (path, bitpix, naxis))
    shape = tuple(int(h["NAXIS%d" % k]) for k in range(naxis, 0, -1))
    a = np.frombuffer(raw, _IMAGE[bitpix], count=int(np.prod(shape))).reshape(shape)
    a = a.astype(a.dtype.newbyteorder("="))
    scale, zero = h.get("BSCALE", 1), h.get("BZERO", 0)
    if scale != 1 or zero != 0:
        a = a.astype(np.float32 if bitpix == 16 else np.float64) * scale + zero
    return a


def _table(h, raw, path):
    width, rows, fields = int(h["NAXIS1"]), int(h["NAXIS2"]), int(h["TFIELDS"])
    names, formats, offset, dtype = [], [], 0, []
    for k in range(1, fields + 1):
        form = str(h["TFORM%d" % k]).strip()
        repeat, code = form[:-1], form[-1:]
        if code not in _COLUMN or repeat not in ("", "1"):
            raise IOError("fits_lite: column %d of %s has the format %r; scalar E, D, J and K columns are read (install astropy "
                          "for the rest)" % (k, path, form))
        name = str(h.get("TTYPE%d" % k, "col%d" % k)).strip()
        names.append(name)
        dtype.append((name, _COLUMN[code]))
        offset += np.dtype(_COLUMN[code]).itemsize
    if offset != width:
        raise IOError("fits_lite: the columns of %s take %d bytes of a row of %d" % (path, offset, width))
    rec = np.frombuffer(raw, np.dtype(dtype), count=rows)
    return {n: rec[n].astype(rec[n].dtype.newbyteorder("=")) for n in names}


def _getdata(path, ext):
    with open(path, "rb") as f:
        k = 0
        while True:
            if k > 0 and not f.read(1):
                raise IOError("fits_lite: %s has no HDU %d" % (path, ext))
            if k > 0:
                f.seek(-1, 1)
            h = _read_header(f, path)
            n = _data_bytes(h)
            if k == ext:
                raw = f.read(n)
                if len(raw) < n:
                    raise IOError("fits_lite: %s ends inside the data of HDU %d" % (path, ext))
                if k == 0 or h.get("XTENSION") == "IMAGE":
                    return _image(h, raw, path)
                if h.get("XTENSION") == "BINTABLE":
                    return _table(h, raw, path)
                raise IOError("fits_lite: HDU %d of %s is a %r extension; images and BINTABLE are read" % (ext, path,
                                                                                                       h.get("XTENSION")))
            f.seek((n + BLOCK - 1) // BLOCK * BLOCK, 1)
            k += 1


def getdata(path, ext=0, force_lite=False):
    """the data of HDU `ext`: an array for an image, {column name: array} (or astropy's record array, which is indexed by
    name in the same way) for a binary table"""
    if not force_lite:
        try:
            from astropy.io import fits
        except ImportError:
            fits = None
        if fits is not None:
            return fits.getdata(path, ext)
    return _getdata(str(path), int(ext))
