// hole_fill_ref.cc — CPU restatement, in our own words, of what a reference user computes when filling the holes of a
// masked image: grassfire (src/vw/Image/Grassfire.h:79-228), the blob index over the whole image as one tile
// (Image/BlobIndex.h:113-306, :385-477), get_blob_sizes (:507-615), ErodeView (Image/ErodeView.h:199-221), InpaintView
// (Image/InpaintView.h:44-237), fill_holes_grass (:239-311) and fill_nodata_with_avg (:317-387).  Test infrastructure
// only: serial, one pixel at a time, in the reference's order of operations.
//
// Pixel kinds: 0 = uint8 mask (non-zero = valid), 1 = PixelMask<float> {value, valid}, 2 / 3 = PixelMask<Vector2i> /
// PixelMask<Vector2f> {dx, dy, valid}; the validity word of a float kind is a float compared with 0.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

enum { KIND_U8 = 0, KIND_MASKED_F32 = 1, KIND_DISP_I32 = 2, KIND_DISP_F32 = 3 };
enum { EDGE_REFERENCE = 0, EDGE_FIXED = 1 };

int kind_bytes(int kind) { return kind == KIND_U8 ? 1 : kind == KIND_MASKED_F32 ? 8 : 12; }

bool is_valid(int kind, const void* img, size_t i) {
  switch (kind) {
    case KIND_U8: return static_cast<const uint8_t*>(img)[i] != 0;
    case KIND_MASKED_F32: return static_cast<const float*>(img)[2 * i + 1] != 0.0f;
    case KIND_DISP_I32: return static_cast<const int32_t*>(img)[3 * i + 2] != 0;
    default: return static_cast<const float*>(img)[3 * i + 2] != 0.0f;
  }
}

template <class T>
void grassfire_t(const T* src, int cols, int rows, bool ignore_borders, int32_t* dst) {
  if (cols <= 1 || rows <= 1) {
    std::fill(dst, dst + (size_t)cols * rows, 0);
    return;
  }
  auto S = [&](int x, int y) { return src[(size_t)y * cols + x] == T(); };   // is zero (a NaN is not; -0.0f is)
  auto D = [&](int x, int y) -> int32_t& { return dst[(size_t)y * cols + x]; };
  if (!ignore_borders) {
    // forward: edge pixels are 0 or 1, interior pixels 1 + min(left, up)
    for (int y = 0; y < rows; ++y)
      for (int x = 0; x < cols; ++x) {
        const bool edge = x == 0 || y == 0 || x == cols - 1 || y == rows - 1;
        if (S(x, y)) D(x, y) = 0;
        else if (edge) D(x, y) = 1;
        else D(x, y) = 1 + std::min(D(x - 1, y), D(x, y - 1));
      }
    // backward over the interior: min(right, down) + 1 where that is smaller
    for (int y = rows - 2; y >= 1; --y)
      for (int x = cols - 2; x >= 1; --x)
        if (D(x, y) != 0) {
          const int32_t m = std::min(D(x + 1, y), D(x, y + 1));
          if (m < D(x, y)) D(x, y) = m + 1;
        }
  } else {
    const int32_t cap = cols + rows;
    for (int y = 0; y < rows; ++y)
      for (int x = 0; x < cols; ++x) {
        if (S(x, y)) { D(x, y) = 0; continue; }
        if (y > 0 && x > 0) D(x, y) = std::min(D(x - 1, y), D(x, y - 1)) + 1;
        else if (y > 0) D(x, y) = std::min(cap, D(x, y - 1) + 1);
        else if (x > 0) D(x, y) = std::min(cap, D(x - 1, y) + 1);
        else D(x, y) = cap;
      }
    for (int y = rows - 1; y >= 0; --y)
      for (int x = cols - 1; x >= 0; --x)
        if (D(x, y) != 0) {
          int32_t m = D(x, y);
          if (x < cols - 1) m = std::min(m, D(x + 1, y) + 1);
          if (y < rows - 1) m = std::min(m, D(x, y + 1) + 1);
          D(x, y) = std::min(m, cap);
        }
  }
}

struct Blob {
  int x0, y0, x1, y1;   // half-open box
  int size;
};

// 8-connected components of the selected pixels; the k-th blob is the one whose first pixel in raster order comes k-th.
// labels: 1-based blob number, 0 elsewhere.
void label_blobs(const std::vector<uint8_t>& sel, int w, int h, std::vector<int32_t>* labels, std::vector<Blob>* blobs) {
  labels->assign((size_t)w * h, 0);
  blobs->clear();
  std::vector<int> stack;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      if (!sel[i] || (*labels)[i]) continue;
      const int id = (int)blobs->size() + 1;
      Blob b{x, y, x + 1, y + 1, 0};
      (*labels)[i] = id;
      stack.push_back((int)i);
      while (!stack.empty()) {
        const int p = stack.back();
        stack.pop_back();
        const int px = p % w, py = p / w;
        b.x0 = std::min(b.x0, px); b.y0 = std::min(b.y0, py);
        b.x1 = std::max(b.x1, px + 1); b.y1 = std::max(b.y1, py + 1);
        ++b.size;
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int qx = px + dx, qy = py + dy;
            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
            const size_t q = (size_t)qy * w + qx;
            if (sel[q] && !(*labels)[q]) { (*labels)[q] = id; stack.push_back((int)q); }
          }
      }
      blobs->push_back(b);
    }
}

std::vector<uint8_t> selection(int kind, const void* img, int w, int h, bool invert) {
  std::vector<uint8_t> sel((size_t)w * h);
  for (size_t i = 0; i < sel.size(); ++i) sel[i] = is_valid(kind, img, i) != invert;
  return sel;
}

// the blobs BlobIndexThreaded(.., max_area, ..) keeps, after wipe_big_blobs(wipe) when wipe > 0; labels renumbered
void filter_blobs(int max_area, int wipe, std::vector<int32_t>* labels, std::vector<Blob>* blobs) {
  std::vector<int> renumber(blobs->size() + 1, 0);
  std::vector<Blob> kept;
  for (size_t k = 0; k < blobs->size(); ++k) {
    const Blob& b = (*blobs)[k];
    if (max_area > 0 && b.size > max_area) continue;
    if (wipe > 0 && (b.x1 - b.x0 > wipe || b.y1 - b.y0 > wipe)) continue;
    kept.push_back(b);
    renumber[k + 1] = (int)kept.size();
  }
  for (auto& l : *labels) l = renumber[l];
  blobs->swap(kept);
}

// InpaintTask::operator() for one blob; `in` is the unpatched image, `out` receives the blob's pixels.
// C float channels and a validity word per pixel.
template <int C>
void inpaint_blob(const float* in, int w, int h, const int32_t* labels, int id, const Blob& b, bool use_grassfire,
                  const float* default_px, int semantics, float* out) {
  const int bx0 = b.x0 - 1, by0 = b.y0 - 1, bx1 = b.x1 + 1, by1 = b.y1 + 1;   // grown by one, half-open
  if (semantics == EDGE_REFERENCE ? (bx0 < 0 || by0 < 0 || bx1 >= w || by1 >= h) : (bx0 < 0 || by0 < 0 || bx1 > w || by1 > h)) return;
  const int pw = bx1 - bx0, ph = by1 - by0;
  std::vector<uint8_t> mask((size_t)pw * ph, 0);
  std::vector<float> patch((size_t)pw * ph * C);
  for (int j = 0; j < ph; ++j)
    for (int i = 0; i < pw; ++i) {
      const size_t g = (size_t)(by0 + j) * w + (bx0 + i);
      mask[(size_t)j * pw + i] = labels[g] == id ? 255 : 0;
      for (int c = 0; c < C; ++c) patch[((size_t)j * pw + i) * C + c] = in[g * (C + 1) + c];
    }
  if (use_grassfire) {
    std::vector<int32_t> dist((size_t)pw * ph);
    grassfire_t<uint8_t>(mask.data(), pw, ph, false, dist.data());
    const int max_distance = *std::max_element(dist.begin(), dist.end());
    std::vector<int> order;
    for (int d = 1; d <= max_distance; ++d)
      for (int i = 0; i < pw; ++i)
        for (int j = 0; j < ph; ++j)
          if (dist[(size_t)j * pw + i] == d) order.push_back(j * pw + i);
    static const double W8[8] = {.176765, .073235, .176765, .073235, .073235, .176765, .073235, .176765};
    const int off[8] = {-pw - 1, -pw, -pw + 1, -1, 1, pw - 1, pw, pw + 1};
    for (int sweep = 0; sweep < 10 * max_distance * max_distance; ++sweep)
      for (int p : order)
        for (int c = 0; c < C; ++c) {
          float sum = 0.0f;
          for (int k = 0; k < 8; ++k) sum = (float)((double)sum + W8[k] * (double)patch[(size_t)(p + off[k]) * C + c]);
          patch[(size_t)p * C + c] = sum;
        }
  }
  for (int j = 0; j < ph; ++j)
    for (int i = 0; i < pw; ++i) {
      if (!mask[(size_t)j * pw + i]) continue;
      float* o = out + ((size_t)(by0 + j) * w + (bx0 + i)) * (C + 1);
      if (use_grassfire) {
        for (int c = 0; c < C; ++c) o[c] = patch[((size_t)j * pw + i) * C + c];
        o[C] = 1.0f;
      } else {
        for (int c = 0; c <= C; ++c) o[c] = default_px[c];
      }
    }
}

int inpaint_all(int kind, const void* img, int w, int h, const std::vector<int32_t>& labels, const std::vector<Blob>& blobs,
                bool use_grassfire, const float* default_px, int semantics, void* out) {
  if (kind != KIND_MASKED_F32 && kind != KIND_DISP_F32) return -1;
  if (out != img) std::memcpy(out, img, (size_t)w * h * kind_bytes(kind));
  std::vector<float> in(static_cast<const float*>(img), static_cast<const float*>(img) + (size_t)w * h * (kind == KIND_MASKED_F32 ? 2 : 3));
  for (size_t k = 0; k < blobs.size(); ++k) {
    if (kind == KIND_MASKED_F32)
      inpaint_blob<1>(in.data(), w, h, labels.data(), (int)k + 1, blobs[k], use_grassfire, default_px, semantics, static_cast<float*>(out));
    else
      inpaint_blob<2>(in.data(), w, h, labels.data(), (int)k + 1, blobs[k], use_grassfire, default_px, semantics, static_cast<float*>(out));
  }
  return 0;
}

}  // namespace

extern "C" {

// src_type: 0 = uint8, 1 = int32, 2 = float
int hfr_grassfire(int src_type, const void* src, int w, int h, int ignore_borders, int32_t* dst) {
  if (w <= 0 || h <= 0) return -1;
  switch (src_type) {
    case 0: grassfire_t(static_cast<const uint8_t*>(src), w, h, ignore_borders != 0, dst); return 0;
    case 1: grassfire_t(static_cast<const int32_t*>(src), w, h, ignore_borders != 0, dst); return 0;
    case 2: grassfire_t(static_cast<const float*>(src), w, h, ignore_borders != 0, dst); return 0;
  }
  return -1;
}

// table: {min.x, min.y, max.x, max.y, size} per kept blob (optional).  Returns -6 with *count set when cap is too small.
int hfr_blob_index(int kind, const void* img, int w, int h, int invert, int max_area, int wipe, int32_t* labels, int32_t* table,
                   int cap, int* count) {
  if (w <= 0 || h <= 0 || kind < 0 || kind > 3) return -1;
  std::vector<int32_t> lab;
  std::vector<Blob> blobs;
  label_blobs(selection(kind, img, w, h, invert != 0), w, h, &lab, &blobs);
  filter_blobs(max_area, wipe, &lab, &blobs);
  *count = (int)blobs.size();
  if (labels) std::copy(lab.begin(), lab.end(), labels);
  if (table) {
    if (cap < (int)blobs.size()) return -6;
    for (size_t k = 0; k < blobs.size(); ++k) {
      const Blob& b = blobs[k];
      const int32_t row[5] = {b.x0, b.y0, b.x1, b.y1, b.size};
      std::copy(row, row + 5, table + 5 * k);
    }
  }
  return 0;
}

int hfr_blob_sizes(int kind, const void* img, int w, int h, uint32_t limit, uint32_t* out) {
  if (w <= 0 || h <= 0 || kind < 0 || kind > 3) return -1;
  std::vector<int32_t> lab;
  std::vector<Blob> blobs;
  label_blobs(selection(kind, img, w, h, false), w, h, &lab, &blobs);
  for (size_t i = 0; i < lab.size(); ++i) out[i] = lab[i] ? std::min((uint32_t)blobs[lab[i] - 1].size, limit) : 0u;
  return 0;
}

// ErodeView over the blobs of valid pixels with size <= max_area: their pixels become the default pixel (all words 0)
int hfr_erode_blobs(int kind, const void* img, int w, int h, int max_area, void* out) {
  if (w <= 0 || h <= 0 || kind < 0 || kind > 3) return -1;
  std::vector<int32_t> lab;
  std::vector<Blob> blobs;
  label_blobs(selection(kind, img, w, h, false), w, h, &lab, &blobs);
  const int nb = kind_bytes(kind);
  if (out != img) std::memcpy(out, img, (size_t)w * h * nb);
  for (size_t i = 0; i < lab.size(); ++i)
    if (lab[i] && blobs[lab[i] - 1].size <= max_area) std::memset(static_cast<char*>(out) + i * nb, 0, nb);
  return 0;
}

// InpaintView over a blob selection {labels, table, count} as hfr_blob_index returned it
int hfr_inpaint(int kind, const void* img, int w, int h, const int32_t* labels, const int32_t* table, int count, int use_grassfire,
                const float* default_px, int semantics, void* out) {
  if (w <= 0 || h <= 0) return -1;
  std::vector<int32_t> lab(labels, labels + (size_t)w * h);
  std::vector<Blob> blobs(count);
  for (int k = 0; k < count; ++k) blobs[k] = Blob{table[5 * k], table[5 * k + 1], table[5 * k + 2], table[5 * k + 3], table[5 * k + 4]};
  return inpaint_all(kind, img, w, h, lab, blobs, use_grassfire != 0, default_px, semantics, out);
}

// fill_holes_grass(img, len) rasterised in one call over the whole image
int hfr_fill_holes_grass(int kind, const void* img, int w, int h, int len, int semantics, void* out) {
  if (w <= 0 || h <= 0 || len < 0) return -1;
  std::vector<int32_t> lab;
  std::vector<Blob> blobs;
  label_blobs(selection(kind, img, w, h, true), w, h, &lab, &blobs);
  filter_blobs(len * len, 0, &lab, &blobs);
  // wipe_big_blobs(len): every blob wider or taller than len goes, also for len == 0
  {
    std::vector<int> renumber(blobs.size() + 1, 0);
    std::vector<Blob> kept;
    for (size_t k = 0; k < blobs.size(); ++k)
      if (blobs[k].x1 - blobs[k].x0 <= len && blobs[k].y1 - blobs[k].y0 <= len) { kept.push_back(blobs[k]); renumber[k + 1] = (int)kept.size(); }
    for (auto& l : lab) l = renumber[l];
    blobs.swap(kept);
  }
  const float zero[3] = {0.0f, 0.0f, 0.0f};
  return inpaint_all(kind, img, w, h, lab, blobs, true, zero, semantics, out);
}

// FillNoDataWithAvg::operator() on PixelMask<float> {value, valid}
int hfr_fill_nodata_with_avg(const float* img, int w, int h, int kernel_size, float* out) {
  if (w <= 0 || h <= 0 || kernel_size <= 0 || kernel_size % 2 == 0) return -1;
  const int k2 = kernel_size / 2;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      float val = img[2 * i], v = img[2 * i + 1];
      if (v == 0.0f) {
        float sum = 0.0f;
        int n = 0;
        for (int c = std::max(0, x - k2); c <= std::min(w - 1, x + k2); ++c)
          for (int r = std::max(0, y - k2); r <= std::min(h - 1, y + k2); ++r) {
            const size_t q = (size_t)r * w + c;
            if (img[2 * q + 1] == 0.0f) continue;
            sum += img[2 * q];
            ++n;
          }
        if (n) { val = sum / (float)n; v = 1.0f; }
      }
      out[2 * i] = val;
      out[2 * i + 1] = v;
    }
  return 0;
}

}  // extern "C"
