"""The lossless PNG stream of the folder driver's frames, stated in integers (the definition rib_png is bit-equal to).

encode_host(u8_hwc) -> bytes states every byte of the file of one uint8 [H, W, 3] frame, 1 <= W <= 4096, 1 <= H <= 65535.
The stream and the tables are this project's; every standard decoder reads the file.  It is built so that a GPU workgroup per
strip can write it without an LZ77 search, without building a Huffman tree and without a checksum that spans workgroups:

  container  signature, IHDR (8 bit, colour type 2, no interlace), one IDAT chunk with the zlib header 78 01, one IDAT chunk
             per strip, one IDAT chunk with the Adler-32 of the whole filtered image, IEND.  A zlib stream may be cut into
             IDAT chunks anywhere; cut at the strip ends, every chunk CRC is a strip's own business.
  strip      STRIP_ROWS = 8 image rows (the last strip may be shorter): per row a filter-type byte and 3 W filtered bytes,
             n = rows * (1 + 3 W) bytes.
  filter     per row the one of None, Sub, Up, Average (floor), Paeth (ties a, b, c) with the smallest sum of |int8(byte)|
             over the row's 3 W filtered bytes, a tie going to the lower type; bpp = 3, bytes left of the row and above
             row 0 are zero, and "above" is always the RAW row, so strips depend on each other's input only.
  tokens     the strip's n bytes cut into maximal runs of equal bytes; a run of R: one literal, then with m = R - 1, while
             m >= 4 a match of length min(m, 258) at distance 1, then m literals.  No other match exists; the only distance
             symbol is code 0 and no match reaches outside its strip.
  code       one dynamic-Huffman block per strip whose literal/length code is TABLES[k], the k that minimises
             header_bits[k] + sum(hist * TABLES[k]) (hist counts end-of-block too; a tie goes to the lower k); the single
             distance code has length 1.  The block header per table (table_header) is fixed, so it is a precomputed bit
             string: BTYPE = 10, HLIT = 29, HDIST = 0, HCLEN, the code-length code, the 286 + 1 lengths run-length coded with
             the symbols 16 - 18 (cl_symbols) under the cheapest code of at most 7 bits (cl_code_lengths).
  bits       BFINAL (1 only for the last strip), the header, the tokens (a literal code, or a length code, its extra bits and
             the one-bit distance code 0), end-of-block; a strip that is not the last appends an empty stored block (000, zero
             bits to the byte boundary, 00 00 FF FF), the last strip pads with zero bits: every strip is whole bytes.
  checksums  each chunk's CRC is zlib.crc32 of its type and data; the Adler-32 is zlib.adler32 of all filtered bytes.

The compression is run-length plus table-selected Huffman: a file is typically the size of zlib level 1, larger than level 6
on smooth content and larger than level 1 on flat graphics.  tools/png_tables.py generated TABLES.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
STRIP_ROWS = 8
MAX_W = 4096
MAX_H = 65535
NSYM = 286
MAX_TABLES = 16
HEADER_BITS_BOUND = 17 + 19 * 3 + 287 * 7      # BTYPE .. HCLEN, the code-length code, 287 lengths of at most 7 bits (16 - 18 only save)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

TABLES = np.array([
    [8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8,
     8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8,
     8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 8,
     8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8,
     8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8,
     8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9],
    [1, 3, 5, 8, 10, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 9, 6, 4, 2, 13, 15, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 12],
    [1, 3, 5, 7, 10, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 9, 7, 5, 3, 15, 15, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8, 8, 8, 9, 9, 9, 9, 10, 15, 15, 15, 15, 15, 15, 15, 5],
    [1, 3, 4, 5, 6, 7, 9, 11, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 14, 10, 8, 7, 6, 5, 4, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15],
    [1, 3, 4, 6, 7, 8, 9, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 9, 8, 7, 6, 4, 3, 15, 15, 7, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 10, 11, 12, 12, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 6],
    [2, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 10, 12, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 12, 11, 9, 9, 8, 8, 7, 7, 6, 6, 5, 5, 4, 4, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15],
    [2, 3, 4, 4, 5, 6, 6, 7, 8, 8, 9, 9, 10, 11, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 10, 10, 9, 9, 8, 7, 7, 6, 6, 5, 4, 4, 3, 15, 15, 7, 7, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10, 10, 15, 15, 15, 15, 15, 15, 15, 15, 15, 6],
    [3, 4, 4, 4, 5, 5, 5, 5, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8, 9, 9, 9, 9, 10, 10, 10, 11, 11, 12, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 11, 11, 11, 10, 10, 10, 9, 9, 9, 9, 8,
     8, 8, 7, 7, 7, 6, 6, 6, 6, 5, 5, 5, 4, 4, 4, 4, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 14],
    [2, 4, 4, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 8, 8, 8, 8, 9, 9, 9, 9, 10, 10, 10, 11, 11, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 13, 11, 11, 10, 10, 10, 9, 9, 9, 9,
     8, 8, 8, 8, 7, 7, 7, 6, 6, 6, 6, 5, 5, 5, 4, 4, 15, 15, 7, 7, 7, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 11, 11, 12, 15, 15, 15, 15, 15, 6],
    [4, 4, 5, 5, 5, 5, 5, 5, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11,
     11, 12, 12, 12, 12, 12, 12, 12, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 12, 12, 12, 12, 12, 12, 12, 11, 11, 11, 11, 11, 11, 10, 10, 10, 10, 10, 10, 10, 9, 9, 9, 9, 9, 9, 9, 8, 8, 8, 8, 8, 8, 8, 7, 7, 7, 7, 7,
     7, 7, 6, 6, 6, 6, 6, 6, 6, 5, 5, 5, 5, 5, 5, 4, 14, 15, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 11],
    [3, 5, 5, 5, 5, 5, 5, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11,
     12, 12, 12, 12, 12, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 12, 12, 12, 12, 12, 11, 11, 11, 11, 11, 11, 11, 10, 10, 10, 10, 10, 10, 10, 9, 9, 9, 9, 9, 9, 8, 8, 8, 8, 8, 8, 8, 8, 7, 7, 7,
     7, 7, 7, 6, 6, 6, 6, 6, 6, 6, 5, 5, 5, 5, 5, 5, 13, 15, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10, 11, 11, 11, 11, 12, 12, 13, 6],
    [5, 5, 5, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9,
     9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12,
     12, 12, 12, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14,
     13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 10, 10, 10, 10, 10, 10, 10,
     10, 10, 10, 10, 10, 10, 10, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7,
     7, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 5, 5, 12, 15, 12, 13, 13, 13, 13, 13, 13, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 11],
    [3, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 9,
     9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12,
     13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14,
     14, 14, 14, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 10, 10, 10,
     10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7,
     7, 7, 7, 7, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 12, 15, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 10, 10, 10, 10, 11, 11, 11, 11, 11, 12, 12, 12, 6],
    [1, 5, 7, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 7, 5, 15, 15, 5, 5, 5, 5, 5, 5, 5, 6, 6, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8, 8, 8, 9, 10, 10, 15, 15, 15, 4],
], dtype=np.uint8)


# ---- deflate's length symbols (RFC 1951 3.2.5) ----
_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def _length_tables():
    sym = np.zeros(259, np.int32)
    ebits = np.zeros(259, np.int32)
    eval_ = np.zeros(259, np.int32)
    for length in range(3, 259):
        s = max(i for i in range(29) if _LEN_BASE[i] <= length)
        if length == 258:
            s = 28
        sym[length], ebits[length], eval_[length] = 257 + s, _LEN_EXTRA[s], length - _LEN_BASE[s]
    return sym, ebits, eval_


LEN_SYM, LEN_EBITS, LEN_EVAL = _length_tables()


def check_tables(tables):
    """Raise unless `tables` is uint8 [K, 286], 1 <= K <= 16, every table complete with lengths 1..15 and table 0 flat."""
    t = np.asarray(tables)
    if t.dtype != np.uint8 or t.ndim != 2 or t.shape[1] != NSYM or not 1 <= t.shape[0] <= MAX_TABLES:
        raise ValueError("code tables must be uint8 [K, 286] with 1 <= K <= 16")
    if t.min() < 1 or t.max() > 15:
        raise ValueError("every code length must lie in 1..15")
    kraft = (1 << (15 - t.astype(np.int64))).sum(axis=1)
    if (kraft != 1 << 15).any():
        raise ValueError("table %d is not a complete prefix code" % int(np.flatnonzero(kraft != 1 << 15)[0]))
    if t[0].max() > 9:
        raise ValueError("table 0 must be flat: every length at most 9")


def canonical_codes(lengths):
    """RFC 1951 3.2.2: the code of every symbol from the code lengths (0: unused)."""
    lengths = [int(l) for l in lengths]
    maxl = max(lengths)
    count = [0] * (maxl + 2)
    for l in lengths:
        if l:
            count[l] += 1
    code, nxt = 0, [0] * (maxl + 2)
    for bits in range(1, maxl + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        out.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return out


def reverse_bits(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def cl_symbols(lengths):
    """The 287 code lengths as (symbol, extra bits, extra value) of the code-length alphabet: a run of c zeros takes 18
    (11..138) while c >= 11, then 17 (3..10) while c >= 3, then single zeros; a run of c equal non-zero lengths takes the
    length once, then 16 (3..6) while c >= 3, then single lengths."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v = int(lengths[i])
        c = 1
        while i + c < n and int(lengths[i + c]) == v:
            c += 1
        i += c
        if v == 0:
            while c >= 11:
                r = min(c, 138)
                out.append((18, 7, r - 11))
                c -= r
            while c >= 3:
                r = min(c, 10)
                out.append((17, 3, r - 3))
                c -= r
        else:
            out.append((v, 0, 0))
            c -= 1
            while c >= 3:
                r = min(c, 6)
                out.append((16, 2, r - 3))
                c -= r
        out.extend([(v, 0, 0)] * c)
    return out


def cl_code_lengths(freq, limit=7):
    """The cheapest complete prefix code of at most `limit` bits for the used symbols of the 19-symbol code-length alphabet:
    the used symbols sorted by (-freq, symbol) take non-decreasing lengths, and a search over the number of leaves per level
    (level 1 first, the smaller count first, a strictly smaller cost wins) picks the counts.  At least two symbols are used."""
    used = sorted((s for s in range(19) if freq[s]), key=lambda s: (-freq[s], s))
    u = len(used)
    f = [freq[s] for s in used]
    inf = 1 << 60
    memo = {}

    def best(level, i, avail):                # symbols i.. on levels level..limit with `avail` open nodes: (cost, leaves here)
        rem = u - i
        if avail > rem or rem > avail << (limit - level):
            return inf, 0
        if level == limit:
            return level * sum(f[i:]), rem    # avail == rem here
        key = (level, i, avail)
        if key not in memo:
            res = (inf, 0)
            for n in range(0, min(avail, rem) + 1):
                if n == rem and n != avail:
                    continue
                c = best(level + 1, i + n, 2 * (avail - n))[0] if n < rem else 0
                if c >= inf:
                    continue
                c += level * sum(f[i:i + n])
                if c < res[0]:
                    res = (c, n)
            memo[key] = res
        return memo[key]

    lengths = [0] * 19
    level, i, avail = 1, 0, 2
    while i < u:
        n = best(level, i, avail)[1]
        for s in used[i:i + n]:
            lengths[s] = level
        i, avail, level = i + n, 2 * (avail - n), level + 1
    return lengths


def table_header(lengths):
    """The dynamic-block header of one table, without the BFINAL bit, as a uint8 array of bits in stream order."""
    syms = cl_symbols([int(l) for l in lengths] + [1])             # 286 literal/length lengths, one distance length
    freq = [0] * 19
    for s, _, _ in syms:
        freq[s] += 1
    cl = cl_code_lengths(freq)
    codes = canonical_codes(cl)
    hclen = max(i for i in range(19) if cl[CL_ORDER[i]]) + 1
    hclen = max(hclen, 4)
    fields = [(2, 2), (29, 5), (0, 5), (hclen - 4, 4)] + [(cl[CL_ORDER[i]], 3) for i in range(hclen)]
    for s, eb, ev in syms:
        fields.append((reverse_bits(codes[s], cl[s]), cl[s]))
        if eb:
            fields.append((ev, eb))
    bits = []
    for v, n in fields:
        bits.extend((v >> b) & 1 for b in range(n))
    return np.array(bits, np.uint8)


class Coder:
    """Everything fixed by a set of tables: reversed codes, headers, the price of a header."""

    def __init__(self, tables):
        check_tables(tables)
        self.tables = np.asarray(tables).astype(np.int64)
        self.K = self.tables.shape[0]
        self.headers = [table_header(t) for t in self.tables]
        self.header_bits = np.array([h.size for h in self.headers], np.int64)
        assert self.header_bits.max() <= HEADER_BITS_BOUND
        self.rcodes = np.array([[reverse_bits(c, int(l)) for c, l in zip(canonical_codes(t), t)] for t in self.tables], np.int64)


_coder = None


def coder():
    global _coder
    if _coder is None:
        _coder = Coder(TABLES)
    return _coder


def strip_bound(n):
    """Upper bound of one strip's IDAT chunk (see max_bytes)."""
    return 12 + (1 + HEADER_BITS_BOUND + 9 * n + 9 + 10 + 7) // 8 + 4


def max_bytes(H, W):
    """An upper bound of one file, derived from the flat table 0.

    A strip takes the cheapest table, so it costs no more than under table 0, whose 286 lengths are all <= 9: a literal costs
    at most 9 bits per byte, a match at most 9 + 5 + 1 bits (length code, extra bits, distance code) for four or more bytes,
    i.e. less than 9 bits per byte too; so the n bytes of a strip cost at most 9 n bits.  Around them: BFINAL (1), the header
    (at most max_header_bits = HEADER_BITS_BOUND, which holds for every set of tables, so that the bound depends on (H, W)
    only), end-of-block (9), the stored block's three bits and the padding (10), its four length bytes, and the chunk's
    length, type and CRC (12): 12 + ceil((1 + max_header_bits + 9 n + 9 + 10) / 8) + 4 bytes.  The prefix
    (signature 8, IHDR 25, the zlib header's chunk 14), the Adler chunk (16) and IEND (12) are added to the sum over strips.
    encode_host asserts the bound."""
    if not (1 <= W <= MAX_W and 1 <= H <= MAX_H):
        raise ValueError("png: H=%d W=%d: 1 <= H <= 65535, 1 <= W <= 4096" % (H, W))
    full, last = divmod(H, STRIP_ROWS)
    total = 47 + 16 + 12 + full * strip_bound(STRIP_ROWS * (1 + 3 * W))
    if last:
        total += strip_bound(last * (1 + 3 * W))
    return total


def filter_rows(img):
    """img uint8 [H, W, 3] -> (filtered uint8 [H, 1 + 3 W] with the type in column 0, costs int64 [H, 5])."""
    H, W, _ = img.shape
    raw = img.reshape(H, 3 * W).astype(np.int32)
    a = np.zeros_like(raw)
    a[:, 3:] = raw[:, :-3]
    b = np.zeros_like(raw)
    b[1:] = raw[:-1]
    c = np.zeros_like(raw)
    c[:, 3:] = b[:, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([raw, raw - a, raw - b, raw - ((a + b) >> 1), raw - paeth]) & 255          # [5, H, 3W]
    costs = np.where(cand >= 128, 256 - cand, cand).sum(axis=2).T.astype(np.int64)              # [H, 5]
    ftype = np.argmin(costs, axis=1)                                                            # the first minimum: the lower type
    out = np.empty((H, 1 + 3 * W), np.uint8)
    out[:, 0] = ftype
    out[:, 1:] = cand[ftype, np.arange(H)]
    return out, costs


def strip_tokens(d):
    """The tokens of one strip's bytes d (uint8, 1-D), in order: (symbol, length) with length 0 for a literal."""
    n = d.size
    starts = np.flatnonzero(np.concatenate(([True], d[1:] != d[:-1])))
    R = np.diff(np.concatenate((starts, [n])))
    m = R - 1
    full = m // 258
    r = m - 258 * full
    rem = (r >= 4).astype(np.int64)
    tail = np.where(r >= 4, 0, r)
    cnt = 1 + full + rem + tail
    run = np.repeat(np.arange(starts.size), cnt)
    j = np.arange(run.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    length = np.where((j >= 1) & (j <= full[run]), 258, np.where((j == full[run] + 1) & (rem[run] == 1), r[run], 0))
    sym = np.where(length > 0, LEN_SYM[length], d[starts][run])
    return sym.astype(np.int64), length.astype(np.int64)


def pack_bits(vals, nbits):
    """Fields of at most 24 bits, least significant bit first, as a uint8 array of bits in stream order."""
    vals = np.asarray(vals, np.int64)
    nbits = np.asarray(nbits, np.int64)
    k = np.arange(24)
    bits = ((vals[:, None] >> k) & 1).astype(np.uint8)
    return bits[k[None, :] < nbits[:, None]]


def encode_strip(d, last, cd=None):
    """One strip's bytes of the zlib stream (whole bytes) and the table it chose."""
    cd = cd or coder()
    sym, length = strip_tokens(d)
    hist = np.bincount(sym, minlength=NSYM).astype(np.int64)
    hist[256] += 1
    cost = cd.header_bits + (cd.tables * hist[None, :]).sum(axis=1)
    k = int(np.argmin(cost))                                   # the first minimum: the lower k
    code, clen = cd.rcodes[k], cd.tables[k]
    eb = LEN_EBITS[length]
    is_match = length > 0
    vals = code[sym] | np.where(is_match, LEN_EVAL[length].astype(np.int64) << clen[sym], 0)     # the distance code 0 follows as a zero bit
    nb = clen[sym] + np.where(is_match, eb + 1, 0)
    parts = [np.array([1 if last else 0], np.uint8), cd.headers[k], pack_bits(vals, nb), pack_bits([code[256]], [clen[256]])]
    nbit = sum(p.size for p in parts)
    assert nbit == 1 + cost[k] + int(np.where(is_match, eb + 1, 0).sum())      # the extra and distance bits are the same under every table
    if not last:
        nbit += 3
    pad = -nbit % 8
    parts.append(np.zeros((0 if last else 3) + pad, np.uint8))
    out = np.packbits(np.concatenate(parts), bitorder="little").tobytes()
    if not last:
        out += b"\x00\x00\xff\xff"
    return out, k


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def prefix(H, W):
    """Signature, IHDR and the IDAT chunk of the zlib header: what depends on (H, W) only."""
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", b"\x78\x01")


def encode_host(u8_hwc, tables=None, info=None):
    """The file of one uint8 [H, W, 3] frame.  info, a dict, receives 'filters' (per row) and 'tables' (per strip)."""
    img = np.ascontiguousarray(u8_hwc)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("encode_host takes a uint8 [H, W, 3] frame")
    H, W, _ = img.shape
    bound = max_bytes(H, W)
    cd = coder() if tables is None else Coder(tables)
    filtered, _ = filter_rows(img)
    out = [prefix(H, W)]
    chosen = []
    for y0 in range(0, H, STRIP_ROWS):
        d = filtered[y0:y0 + STRIP_ROWS].reshape(-1)
        data, k = encode_strip(d, y0 + STRIP_ROWS >= H, cd)
        assert 12 + len(data) <= strip_bound(d.size)
        chosen.append(k)
        out.append(chunk(b"IDAT", data))
    out.append(chunk(b"IDAT", struct.pack(">I", zlib.adler32(filtered.tobytes()) & 0xFFFFFFFF)))
    out.append(chunk(b"IEND", b""))
    data = b"".join(out)
    assert len(data) <= bound
    if info is not None:
        info["filters"] = filtered[:, 0].copy()
        info["tables"] = chosen
    return data
