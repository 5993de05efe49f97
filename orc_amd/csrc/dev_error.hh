// Device-side error codes, their reference texts and statuses. No HIP: the
// host stream planners (host_plan.hh) report with the same codes.
#pragma once

#include <stdint.h>

#include "../../include/orcg.h"

namespace orcg {

// Device-side error codes (the low byte of the packed device error record).
// Messages are the reference's ParseError texts (c++/src/RleDecoderV2.cc).
enum DevErr : uint32_t {
  kErrNone = 0,
  kErrBadRead = 1,         // "bad read in RleDecoderV2::readByte"            :38
  kErrPatchedPl0 = 2,      // "Corrupt PATCHED_BASE encoded data (pl==0)!"     :307
  kErrPatchedWidth = 3,    // "... (patchBitSize + pgw > 64)!"                 :328-330
  kErrDeltaLength = 4,     // "Illegal run length for delta encoding: 1"       :412-415
  kErrBadSegment = 5,      // positions / segment table not run aligned (InvalidArgument)
  kErrByteBadRead = 6,     // "bad read in nextBuffer" (ByteRLE.cc:364)
  kErrDictIndex = 7,       // "Entry index out of range in StringDictionaryColumn" (ColumnReader.cc:578)
  kErrV1BadRead = 8,       // "bad read in readByte" (RLEv1.cc:141-146)
  kErrDecimalScale = 9,    // "Decimal scale out of range" (ColumnReader.cc:1348)
  kErrHive11Overflow = 10, // "Hive 0.11 decimal was more than 38 digits." (ColumnReader.cc:1654)
  // Java face (RunLengthIntegerReaderV2.java, readPatchedBaseValues :149-260)
  kErrJavaCorrupt = 11,    // IOException "Corruption in ORC data encountered. ..." (pw + pgw > 64, :196-200)
  kErrJavaPatchIndex = 12, // ArrayIndexOutOfBoundsException: pl == 0 reads unpackedPatch[0] (:207)
  // schema evolution (ConvertColumnReader.cc handleOverflow, :66-76); the caller appends the type names
  kErrConvertOverflow = 13, // "Overflow when convert from <file type> to <read type>"
  // Snappy chunks inflated on the device (inflate_kernels.hip): the texts of the host's
  // snappy_decompress (orc_file.cpp); the record's index is the chunk's table index
  kErrSnappyLiteralTruncated = 14,
  kErrSnappyLiteralRange = 15,
  kErrSnappyCopyTruncated = 16,
  kErrSnappyCopyRange = 17,
  kErrSnappyLength = 18,
  // LZ4 chunks inflated on the device: the host path's one text (decompress_chunk, orc_file.cpp)
  kErrLz4 = 19,
};

inline const char* dev_error_message(uint32_t code) {
  switch (code) {
    case kErrBadRead: return "bad read in RleDecoderV2::readByte";
    case kErrPatchedPl0: return "Corrupt PATCHED_BASE encoded data (pl==0)!";
    case kErrPatchedWidth: return "Corrupt PATCHED_BASE encoded data (patchBitSize + pgw > 64)!";
    case kErrDeltaLength: return "Illegal run length for delta encoding: 1";
    case kErrBadSegment: return "Stream position is not at a run boundary";
    case kErrByteBadRead: return "bad read in nextBuffer";
    case kErrDictIndex: return "Entry index out of range in StringDictionaryColumn";
    case kErrV1BadRead: return "bad read in readByte";
    case kErrDecimalScale: return "Decimal scale out of range";
    case kErrHive11Overflow: return "Hive 0.11 decimal was more than 38 digits.";
    case kErrJavaCorrupt:
      return "Corruption in ORC data encountered. To skip reading corrupted data, set "
             "hive.exec.orc.skip.corrupt.data to true";
    case kErrJavaPatchIndex: return "Index 0 out of bounds for length 0";
    case kErrConvertOverflow: return "Overflow when convert";
    case kErrSnappyLiteralTruncated: return "snappy: truncated literal";
    case kErrSnappyLiteralRange: return "snappy: literal out of range";
    case kErrSnappyCopyTruncated: return "snappy: truncated copy";
    case kErrSnappyCopyRange: return "snappy: copy out of range";
    case kErrSnappyLength: return "snappy: length mismatch";
    case kErrLz4: return "Corrupt lz4 compressed block";
  }
  return "unknown device error";
}

inline int dev_error_status(uint32_t code) {
  return code == kErrBadSegment ? ORCG_INVALID_ARGUMENT : ORCG_PARSE_ERROR;
}

}  // namespace orcg
