// Test driver of "tag AND value" on the class surface (IndexIVF_HNSW::search_batch_tags_values, range_search_tags_values;
// tests/test_gpu_tags_values_class.py builds it with g++).  KIND is ivf (IndexIVF_HNSW) or grouping (IndexIVF_HNSW_Grouping).
//   tags_values_tool KIND d nc code_size nsubc centroids info edges pq norm_pq opq|- in.index queries.fvecs nq k nprobe
//               max_codes ef pruning query_tags.u16 query_ranges.u32 tlabels.u32 tags.u16 vlabels.u32 values.u32
//               add.fvecs|- add_first_id upd.fvecs|- upd_labels.u32 gone.u32 relabels.u32 retags.u16 revalues.u32 out.bin
//               out.index end
//       set_id_tags and set_id_values of the labels in two incremental calls each (no device copy yet: the first search
//       installs them), round, add_batch(add rows, ids add_first_id ..) when given, round, invalidate_device(), round,
//       update_batch(upd rows, upd_labels) when given, round, remove_ids(gone), round, set_id_tags(relabels, retags) and
//       set_id_values(relabels, revalues) on the current copy, round; then: a null tag array must answer as
//       search_batch_values, a null range array as search_batch_tags, the calls must throw while a set_id_filter filter is
//       installed and leave the answers as they were, and after clear_id_tags() + clear_id_values() only the queries whose
//       tag is 0xffff and whose interval reaches 0xffffffff may find anything.  Write.  A round is
//       search_batch_tags_values then range_search_tags_values at radius +inf.
//       out.bin, per round: labels [nq][k] (int64), distances [nq][k] (float), lims [nq + 1] (uint64), range labels
//       [lims[nq]] (int64), range distances [lims[nq]] (float).
// The .u16 / .u32 files are raw arrays; query_ranges.u32 holds lo, hi per query.
#include <ivf-hnsw/IndexIVF_HNSW_Grouping.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ivfhnsw;

template <class T> static std::vector<T> read_raw(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in)
        throw std::runtime_error(std::string("cannot open ") + path);
    in.seekg(0, std::ios::end);
    const size_t n = (size_t)in.tellg() / sizeof(T);
    in.seekg(0);
    std::vector<T> v(n);
    in.read(reinterpret_cast<char *>(v.data()), n * sizeof(T));
    return v;
}

static std::vector<float> read_fvecs(const char *path, size_t d, size_t *n)
{
    std::ifstream bin(path, std::ios::binary);
    if (!bin)
        throw std::runtime_error(std::string("cannot open ") + path);
    bin.seekg(0, std::ios::end);
    *n = (size_t)bin.tellg() / (sizeof(int) + d * sizeof(float));
    bin.seekg(0);
    std::vector<float> x(*n * d);
    readXvec<float>(bin, x.data(), d, *n);
    return x;
}

template <class F> static bool throws(F &&f)
{
    try {
        f();
    } catch (const std::exception &) {
        return true;
    }
    return false;
}

int main(int argc, char **argv)
try {
    typedef IndexIVF_HNSW::idx_t idx_t;
    if (argc != 37 || std::string(argv[36]) != "end")
        throw std::runtime_error("usage: see the head of tags_values_tool.cpp");
    const std::string kind = argv[1];
    const size_t d = atol(argv[2]), nc = atol(argv[3]), cs = atol(argv[4]), nsubc = atol(argv[5]);
    const char *centroids = argv[6], *info = argv[7], *edges = argv[8], *ppq = argv[9], *pnorm = argv[10], *popq = argv[11],
               *pindex = argv[12], *pqueries = argv[13];
    const size_t nq = atol(argv[14]), k = atol(argv[15]), nprobe = atol(argv[16]), max_codes = atol(argv[17]),
                 ef = atol(argv[18]);
    const bool pruning = atoi(argv[19]) != 0;
    const std::vector<uint16_t> qt = read_raw<uint16_t>(argv[20]);
    const std::vector<uint32_t> qr = read_raw<uint32_t>(argv[21]);
    if (qt.size() != nq || qr.size() != 2 * nq)
        throw std::runtime_error("query_tags.u16 must hold nq and query_ranges.u32 2 * nq entries");
    const std::vector<idx_t> tlabels = read_raw<idx_t>(argv[22]);
    const std::vector<uint16_t> tags = read_raw<uint16_t>(argv[23]);
    const std::vector<idx_t> vlabels = read_raw<idx_t>(argv[24]);
    const std::vector<uint32_t> values = read_raw<uint32_t>(argv[25]);
    const char *padd = argv[26];
    const idx_t add_first = (idx_t)atol(argv[27]);
    const char *pupd = argv[28];
    const std::vector<idx_t> upd_labels = read_raw<idx_t>(argv[29]);
    const std::vector<idx_t> gone = read_raw<idx_t>(argv[30]);
    const std::vector<idx_t> relabels = read_raw<idx_t>(argv[31]);
    const std::vector<uint16_t> retags = read_raw<uint16_t>(argv[32]);
    const std::vector<uint32_t> revalues = read_raw<uint32_t>(argv[33]);
    const char *pout = argv[34], *pidx = argv[35];
    if (tlabels.size() != tags.size() || vlabels.size() != values.size() || relabels.size() != retags.size() ||
        relabels.size() != revalues.size())
        throw std::runtime_error("usage: see the head of tags_values_tool.cpp");
    IndexIVF_HNSW *index;
    if (kind == "grouping")
        index = new IndexIVF_HNSW_Grouping(d, nc, cs, 8, nsubc);
    else if (kind == "ivf")
        index = new IndexIVF_HNSW(d, nc, cs, 8);
    else
        throw std::runtime_error("KIND must be ivf or grouping");
    index->build_quantizer(centroids, info, edges, 16, 500);
    index->do_opq = strcmp(popq, "-") != 0;
    delete index->pq;
    index->pq = faiss::read_ProductQuantizer(ppq);
    if (index->do_opq)
        index->opq_matrix = dynamic_cast<faiss::LinearTransform *>(faiss::read_VectorTransform(popq));
    delete index->norm_pq;
    index->norm_pq = faiss::read_ProductQuantizer(pnorm);
    index->read(pindex);
    if (index->do_opq)
        index->rotate_quantizer();
    index->nprobe = nprobe;
    index->max_codes = max_codes;
    index->quantizer->efSearch = ef;
    if (auto *g = dynamic_cast<IndexIVF_HNSW_Grouping *>(index))
        g->do_pruning = pruning;
    std::vector<float> q(nq * d);
    {
        std::ifstream in(pqueries, std::ios::binary);
        readXvec<float>(in, q.data(), d, nq);
    }
    const size_t thalf = tlabels.size() / 2, vhalf = vlabels.size() / 2;
    index->set_id_tags(thalf, tlabels.data(), tags.data());
    index->set_id_values(vhalf, vlabels.data(), values.data());
    index->set_id_tags(tlabels.size() - thalf, tlabels.data() + thalf, tags.data() + thalf);
    index->set_id_values(vlabels.size() - vhalf, vlabels.data() + vhalf, values.data() + vhalf);
    FILE *f = fopen(pout, "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    std::vector<long> lab(nq * k);
    std::vector<float> dist(nq * k);
    auto round = [&]() {
        index->search_batch_tags_values(nq, k, q.data(), qt.data(), qr.data(), dist.data(), lab.data());
        fwrite(lab.data(), sizeof(long), lab.size(), f);
        fwrite(dist.data(), sizeof(float), dist.size(), f);
        std::vector<size_t> lims;
        std::vector<long> rl;
        std::vector<float> rd;
        index->range_search_tags_values(nq, q.data(), qt.data(), qr.data(), INFINITY, lims, rd, rl);
        fwrite(lims.data(), sizeof(size_t), lims.size(), f);
        fwrite(rl.data(), sizeof(long), rl.size(), f);
        fwrite(rd.data(), sizeof(float), rd.size(), f);
    };
    round();
    if (strcmp(padd, "-") != 0) {
        size_t nb;
        const std::vector<float> base = read_fvecs(padd, d, &nb);
        std::vector<idx_t> ids(nb);
        for (size_t i = 0; i < nb; i++)
            ids[i] = add_first + (idx_t)i;
        index->add_batch(nb, base.data(), ids.data());
    }
    round();
    index->invalidate_device(); // the next search uploads everything again, tags and values with it
    round();
    if (strcmp(pupd, "-") != 0) {
        size_t nb;
        const std::vector<float> x = read_fvecs(pupd, d, &nb);
        if (nb != upd_labels.size())
            throw std::runtime_error("upd.fvecs and upd_labels.u32 differ in length");
        index->update_batch(nb, x.data(), upd_labels.data());
    }
    round();
    index->remove_ids(gone.size(), gone.data());
    round();
    index->set_id_tags(relabels.size(), relabels.data(), retags.data());
    index->set_id_values(relabels.size(), relabels.data(), revalues.data());
    round();
    fclose(f);
    const std::vector<long> before = lab;
    // a null array makes the call the other side's
    std::vector<long> other(nq * k);
    index->search_batch_tags_values(nq, k, q.data(), nullptr, qr.data(), dist.data(), lab.data());
    index->search_batch_values(nq, k, q.data(), qr.data(), dist.data(), other.data());
    if (lab != other)
        throw std::runtime_error("search_batch_tags_values without tags differs from search_batch_values");
    index->search_batch_tags_values(nq, k, q.data(), qt.data(), nullptr, dist.data(), lab.data());
    index->search_batch_tags(nq, k, q.data(), qt.data(), dist.data(), other.data());
    if (lab != other)
        throw std::runtime_error("search_batch_tags_values without ranges differs from search_batch_tags");
    // what must throw, leaving the answers as they were
    index->set_id_filter(thalf, tlabels.data());
    if (!throws([&] { index->search_batch_tags_values(nq, k, q.data(), qt.data(), qr.data(), dist.data(), lab.data()); }))
        throw std::runtime_error("search_batch_tags_values with a set_id_filter filter installed did not throw");
    {
        std::vector<size_t> lims;
        std::vector<long> rl;
        std::vector<float> rd;
        if (!throws([&] { index->range_search_tags_values(nq, q.data(), qt.data(), qr.data(), INFINITY, lims, rd, rl); }))
            throw std::runtime_error("range_search_tags_values with a set_id_filter filter installed did not throw");
    }
    index->clear_id_filter();
    index->search_batch_tags_values(nq, k, q.data(), qt.data(), qr.data(), dist.data(), lab.data());
    if (lab != before)
        throw std::runtime_error("the refused calls changed the answers");
    index->clear_id_tags();
    index->clear_id_values();
    index->search_batch_tags_values(nq, k, q.data(), qt.data(), qr.data(), dist.data(), lab.data());
    for (size_t i = 0; i < nq; i++) {
        const bool all = qt[i] == 0xffffu && qr[2 * i] <= qr[2 * i + 1] && qr[2 * i + 1] == 0xffffffffu;
        for (size_t j = 0; j < k; j++)
            if (all != (lab[i * k + j] != -1))
                throw std::runtime_error("after clear_id_tags and clear_id_values only (0xffff, (.., 0xffffffff)) must find its k labels");
    }
    index->write(pidx);
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "tags_values_tool: %s\n", e.what());
    return 1;
}
