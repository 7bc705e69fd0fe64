// Test driver of the row tags of the class surface (IndexIVF_HNSW::set_id_tags, clear_id_tags, search_batch_tags,
// range_search_tags; tests/test_gpu_tags_class.py builds it with g++).  KIND is ivf (IndexIVF_HNSW) or grouping
// (IndexIVF_HNSW_Grouping).
//   tags_tool KIND d nc code_size nsubc centroids info edges pq norm_pq opq|- in.index queries.fvecs nq k nprobe max_codes ef
//             pruning query_tags.u16 labels.u32 tags.u16 add.fvecs|- add_first_id relabels.u32 retags.u16 out.bin out.index
//       set_id_tags of the labels in two incremental calls (no device copy yet: the first search installs them), round,
//       add_batch(add rows, ids add_first_id ..) when given, round, invalidate_device(), round, set_id_tags(relabels,
//       retags) on the current copy, round; then what must throw is tried -- a label given two tags, and a _tags call
//       while a set_id_filter filter is installed -- and clear_id_tags() must leave a tagged query without results.  Write.
//       A round is search_batch_tags then range_search_tags at radius +inf.
//       out.bin, per round: labels [nq][k] (int64), distances [nq][k] (float), lims [nq + 1] (uint64), range labels
//       [lims[nq]] (int64), range distances [lims[nq]] (float).
// labels.u32 / tags.u16 / query_tags.u16 are raw arrays.
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
    if (argc != 30)
        throw std::runtime_error("usage: see the head of tags_tool.cpp");
    const std::string kind = argv[1];
    const size_t d = atol(argv[2]), nc = atol(argv[3]), cs = atol(argv[4]), nsubc = atol(argv[5]);
    const char *centroids = argv[6], *info = argv[7], *edges = argv[8], *ppq = argv[9], *pnorm = argv[10], *popq = argv[11],
               *pindex = argv[12], *pqueries = argv[13];
    const size_t nq = atol(argv[14]), k = atol(argv[15]), nprobe = atol(argv[16]), max_codes = atol(argv[17]),
                 ef = atol(argv[18]);
    const bool pruning = atoi(argv[19]) != 0;
    const std::vector<uint16_t> qtags = read_raw<uint16_t>(argv[20]);
    if (qtags.size() != nq)
        throw std::runtime_error("query_tags.u16 must hold nq entries");
    const std::vector<idx_t> labels = read_raw<idx_t>(argv[21]);
    const std::vector<uint16_t> tags = read_raw<uint16_t>(argv[22]);
    const char *padd = argv[23];
    const idx_t add_first = (idx_t)atol(argv[24]);
    const std::vector<idx_t> relabels = read_raw<idx_t>(argv[25]);
    const std::vector<uint16_t> retags = read_raw<uint16_t>(argv[26]);
    const char *pout = argv[27], *pidx = argv[28];
    if (labels.size() != tags.size() || relabels.size() != retags.size() || std::string(argv[29]) != "end")
        throw std::runtime_error("usage: see the head of tags_tool.cpp");
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
    const size_t half = labels.size() / 2;
    index->set_id_tags(half, labels.data(), tags.data());
    index->set_id_tags(labels.size() - half, labels.data() + half, tags.data() + half);
    FILE *f = fopen(pout, "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    std::vector<long> lab(nq * k);
    std::vector<float> dist(nq * k);
    auto round = [&]() {
        index->search_batch_tags(nq, k, q.data(), qtags.data(), dist.data(), lab.data());
        fwrite(lab.data(), sizeof(long), lab.size(), f);
        fwrite(dist.data(), sizeof(float), dist.size(), f);
        std::vector<size_t> lims;
        std::vector<long> rl;
        std::vector<float> rd;
        index->range_search_tags(nq, q.data(), qtags.data(), INFINITY, lims, rd, rl);
        fwrite(lims.data(), sizeof(size_t), lims.size(), f);
        fwrite(rl.data(), sizeof(long), rl.size(), f);
        fwrite(rd.data(), sizeof(float), rd.size(), f);
    };
    round();
    if (strcmp(padd, "-") != 0) {
        std::ifstream bin(padd, std::ios::binary);
        bin.seekg(0, std::ios::end);
        const size_t nb = (size_t)bin.tellg() / (sizeof(int) + d * sizeof(float));
        bin.seekg(0);
        std::vector<float> base(nb * d);
        readXvec<float>(bin, base.data(), d, nb);
        std::vector<idx_t> ids(nb);
        for (size_t i = 0; i < nb; i++)
            ids[i] = add_first + (idx_t)i;
        index->add_batch(nb, base.data(), ids.data());
    }
    round();
    index->invalidate_device(); // the next search uploads everything again, the tags with it
    round();
    index->set_id_tags(relabels.size(), relabels.data(), retags.data());
    round();
    fclose(f);
    // what must throw, each leaving the tags as they were
    const std::vector<long> before = lab;
    const idx_t twice[2] = {labels[0], labels[0]};
    const uint16_t two_tags[2] = {3, 4};
    if (!throws([&] { index->set_id_tags(2, twice, two_tags); }))
        throw std::runtime_error("a label given two different tags did not throw");
    if (!throws([&] { index->set_id_tags(1, nullptr, two_tags); }))
        throw std::runtime_error("null ids did not throw");
    index->set_id_filter(half, labels.data());
    if (!throws([&] { index->search_batch_tags(nq, k, q.data(), qtags.data(), dist.data(), lab.data()); }))
        throw std::runtime_error("search_batch_tags with a set_id_filter filter installed did not throw");
    {
        std::vector<size_t> lims;
        std::vector<long> rl;
        std::vector<float> rd;
        if (!throws([&] { index->range_search_tags(nq, q.data(), qtags.data(), INFINITY, lims, rd, rl); }))
            throw std::runtime_error("range_search_tags with a set_id_filter filter installed did not throw");
    }
    index->clear_id_filter();
    index->search_batch_tags(nq, k, q.data(), qtags.data(), dist.data(), lab.data());
    if (lab != before)
        throw std::runtime_error("the refused calls changed the answers");
    index->clear_id_tags();
    index->search_batch_tags(nq, k, q.data(), qtags.data(), dist.data(), lab.data());
    for (size_t i = 0; i < nq; i++)
        for (size_t j = 0; j < k; j++)
            if ((qtags[i] != 0xffff) != (lab[i * k + j] == -1))
                throw std::runtime_error("after clear_id_tags a tagged query must find nothing and an untagged one k labels");
    index->write(pidx);
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "tags_tool: %s\n", e.what());
    return 1;
}
