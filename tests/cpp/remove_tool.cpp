// Test driver of IndexIVF_HNSW::remove_ids through the class surface (tests/test_gpu_remove_class.py and
// tests/test_remove_cpu.py build it with g++).  KIND is ivf (IndexIVF_HNSW) or grouping (IndexIVF_HNSW_Grouping).
//   remove_tool host KIND d nc code_size nsubc in.index labels.u32 out.index
//       read, remove_ids(labels), write: the host lists only, no device handle is ever made.  Prints the count removed.
//   remove_tool search KIND d nc code_size nsubc centroids info edges pq norm_pq opq|- in.index queries.fvecs nq k nprobe
//               max_codes ef pruning labels1.u32 labels2.u32 add.fvecs|- add_first_id inplace|reupload out.bin out.index
//       search, remove_ids(labels1), search, add_batch(add rows, ids add_first_id ..) when given, remove_ids(labels2),
//       search, write.  reupload calls invalidate_device() before every change, so remove_ids and add_batch take their
//       host path and the next search uploads the whole index; inplace leaves the class to change the device copy.
//       out.bin: labels [3][nq][k] (int64), distances [3][nq][k] (float), the two removed counts (uint64).
// labels*.u32 are raw uint32 arrays.
#include <ivf-hnsw/IndexIVF_HNSW_Grouping.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ivfhnsw;

static std::vector<IndexIVF_HNSW::idx_t> read_u32(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in)
        throw std::runtime_error(std::string("cannot open ") + path);
    in.seekg(0, std::ios::end);
    const size_t n = (size_t)in.tellg() / sizeof(uint32_t);
    in.seekg(0);
    std::vector<IndexIVF_HNSW::idx_t> v(n);
    in.read(reinterpret_cast<char *>(v.data()), n * sizeof(uint32_t));
    return v;
}

static IndexIVF_HNSW *make_index(const std::string &kind, size_t d, size_t nc, size_t cs, size_t nsubc)
{
    if (kind == "grouping")
        return new IndexIVF_HNSW_Grouping(d, nc, cs, 8, nsubc);
    if (kind != "ivf")
        throw std::runtime_error("KIND must be ivf or grouping");
    return new IndexIVF_HNSW(d, nc, cs, 8);
}

int main(int argc, char **argv)
try {
    if (argc < 2)
        throw std::runtime_error("usage: see the head of remove_tool.cpp");
    const std::string cmd = argv[1];
    if (cmd == "host") {
        if (argc != 10)
            throw std::runtime_error("usage: see the head of remove_tool.cpp");
        IndexIVF_HNSW *index = make_index(argv[2], atol(argv[3]), atol(argv[4]), atol(argv[5]), atol(argv[6]));
        index->read(argv[7]);
        const std::vector<IndexIVF_HNSW::idx_t> lab = read_u32(argv[8]);
        const size_t removed = index->remove_ids(lab.size(), lab.data());
        index->write(argv[9]);
        printf("%zu\n", removed);
        delete index;
        return 0;
    }
    if (cmd != "search" || argc != 28)
        throw std::runtime_error("usage: see the head of remove_tool.cpp");
    const std::string kind = argv[2];
    const size_t d = atol(argv[3]), nc = atol(argv[4]), cs = atol(argv[5]), nsubc = atol(argv[6]);
    const char *centroids = argv[7], *info = argv[8], *edges = argv[9], *ppq = argv[10], *pnorm = argv[11], *popq = argv[12],
               *pindex = argv[13], *pqueries = argv[14];
    const size_t nq = atol(argv[15]), k = atol(argv[16]), nprobe = atol(argv[17]), max_codes = atol(argv[18]),
                 ef = atol(argv[19]);
    const bool pruning = atoi(argv[20]) != 0;
    const std::vector<IndexIVF_HNSW::idx_t> lab1 = read_u32(argv[21]), lab2 = read_u32(argv[22]);
    const char *padd = argv[23];
    const IndexIVF_HNSW::idx_t add_first = (IndexIVF_HNSW::idx_t)atol(argv[24]);
    const std::string mode = argv[25];
    if (mode != "inplace" && mode != "reupload")
        throw std::runtime_error("mode must be inplace or reupload");
    IndexIVF_HNSW *index = make_index(kind, d, nc, cs, nsubc);
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
    std::vector<long> lab(3 * nq * k);
    std::vector<float> dist(3 * nq * k);
    uint64_t removed[2];
    const bool reupload = mode == "reupload";
    index->search_batch(nq, k, q.data(), dist.data(), lab.data());
    if (reupload)
        index->invalidate_device();
    removed[0] = index->remove_ids(lab1.size(), lab1.data());
    index->search_batch(nq, k, q.data(), dist.data() + nq * k, lab.data() + nq * k);
    if (strcmp(padd, "-") != 0) {
        std::ifstream bin(padd, std::ios::binary);
        bin.seekg(0, std::ios::end);
        const size_t nb = (size_t)bin.tellg() / (sizeof(int) + d * sizeof(float));
        bin.seekg(0);
        std::vector<float> base(nb * d);
        readXvec<float>(bin, base.data(), d, nb);
        std::vector<IndexIVF_HNSW::idx_t> ids(nb);
        for (size_t i = 0; i < nb; i++)
            ids[i] = add_first + (IndexIVF_HNSW::idx_t)i;
        if (reupload)
            index->invalidate_device();
        index->add_batch(nb, base.data(), ids.data());
    }
    if (reupload)
        index->invalidate_device();
    removed[1] = index->remove_ids(lab2.size(), lab2.data());
    index->search_batch(nq, k, q.data(), dist.data() + 2 * nq * k, lab.data() + 2 * nq * k);
    FILE *f = fopen(argv[26], "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    fwrite(lab.data(), sizeof(long), lab.size(), f);
    fwrite(dist.data(), sizeof(float), dist.size(), f);
    fwrite(removed, sizeof(uint64_t), 2, f);
    fclose(f);
    index->write(argv[27]);
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "remove_tool: %s\n", e.what());
    return 1;
}
